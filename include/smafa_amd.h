/*
 * smafa_amd.h — C ABI of the MI355X-native smafa scan engine (libsmafa_amd.so).
 *
 * Drop-in boundary for the ONE hot path of wwood/smafa v0.8.0: the fixed-length
 * Hamming scan behind `smafa query` and `smafa cluster`.  The reference has no FFI
 * of its own; each entry point below names the reference code it replaces
 * (file:line relative to the reference tree).  Plain pointers and sizes only — a
 * Rust host binds these 1:1 (see INTEGRATION.md for the `extern "C"` block).
 *
 * Conventions
 *  - every function returns SMAFA_OK (0) or a negative SMAFA_ERR_* code; the text
 *    of the failure (the reference's panic message where there is one) is kept
 *    per thread in smafa_last_error().  Nothing aborts or throws across the ABI.
 *  - sequences cross the boundary as CODE BYTES, one byte per column, row-major
 *    (n rows of seq_len columns), produced by smafa_encode().
 *  - one handle = one owner thread at a time (the reference is single-threaded).
 *  - there is NO CPU fallback: without a HIP device every scan entry point fails
 *    with SMAFA_ERR_DEVICE.
 */
#ifndef SMAFA_AMD_H
#define SMAFA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMAFA_OK 0
#define SMAFA_ERR_INVALID (-1)  /* bad argument */
#define SMAFA_ERR_DEVICE (-2)   /* no HIP device / HIP runtime failure */
#define SMAFA_ERR_CAPACITY (-3) /* caller's hit buffer too small: *n_out = rows needed, grow and retry */
#define SMAFA_ERR_IO (-4)       /* file could not be read / written */
#define SMAFA_ERR_FORMAT (-5)   /* malformed FASTX / DB file, unsupported DB version */
#define SMAFA_ERR_PANIC (-6)    /* input on which the reference panics (message preserved) */
#define SMAFA_ERR_NOMEM (-7)    /* host memory (or threads) ran out inside the call; the handle it was given may only be destroyed */

#define SMAFA_ALPHABET_NT 0 /* A C G T/U N — classes of BYTE_LUT, src/lib.rs:171-178; codes 0..4 */
#define SMAFA_ALPHABET_AA 1 /* build-defined extension: A-Z * - (case-folded), codes 0..27; not in the reference */

#define SMAFA_NONE UINT32_MAX /* "option absent" for max_div / max_num_hits / limit_per_sequence */
#define SMAFA_TAXON_ROOT 0xfffffffeu /* smafa_db_classify: the taxon of a read whose best hits share no rank; no lineage may hold it */

#define SMAFA_DB_VERSION 2u /* CURRENT_DB_VERSION, src/lib.rs:18 */

typedef struct smafa_db smafa_db;     /* subject store resident in HBM — WindowSet, src/lib.rs:54-60 */
typedef struct smafa_qset smafa_qset; /* a packed query batch resident in HBM */
typedef struct smafa_group smafa_group; /* one subject store replicated over several GPUs of a node */

/* one scan result row: the (query_number, i, distance) of src/lib.rs:292 / :310 */
typedef struct {
    uint32_t query;
    uint32_t subject;
    uint32_t dist;
} smafa_hit;

typedef struct {
    uint64_t n_subjects;
    uint32_t seq_len;
    int32_t alphabet;
    int32_t device;
    uint32_t planes;          /* bit-planes stored per subject: 5 (AA), 3 (NT), or 2 (NT store without any N) */
    uint32_t words_per_plane; /* ceil(seq_len / 32) */
    uint64_t hbm_bytes;       /* bytes of the packed subject block in HBM */
    uint64_t bytes_per_subject;
} smafa_db_info_t;

/* state of a store's block index (smafa_db_build_index) */
typedef struct {
    int32_t mode;              /* smafa_set_index */
    int32_t current;           /* 1: an index exists and matches the store as it is now */
    uint32_t blocks;           /* column blocks the index holds: bounds up to blocks - 1 */
    uint32_t usable_blocks;    /* ... of which this many have no run of equal keys too long to probe */
    uint32_t max_div_served;   /* largest bound a big batch is answered from the index at (SMAFA_NONE: none) */
    uint32_t probe_launches;   /* scans of this handle's life that were answered from an index */
    uint64_t bytes;            /* HBM the index occupies */
    uint64_t longest_run;      /* most subjects sharing one block's columns exactly */
    double candidates_per_query; /* subjects a query drawn like the store's rows is compared with at max_div_served */
    double build_ms;
} smafa_index_info_t;

/* ------------------------------------------------------------------ library */
const char *smafa_last_error(void);
int smafa_device_count(void); /* 0 when no MI355X is visible; never fails */
/* Progress / timing lines of the drivers on stderr (the reference logs through env_logger, src/lib.rs:206,230,
 * 320-323; src/cluster.rs:33,87-92): 0 = errors only (--quiet), 1 = info (default of the reference), 2 = debug (-v).
 * The library default is 0 so that stderr stays clean for hosts that do not ask. */
void smafa_set_verbosity(int level);
/* Short hash of the kernel sources this library was built from (recorded beside profiles, so a bench run can tell
 * whether a committed counter profile belongs to the binary it is timing). */
const char *smafa_build_id(void);
/* Measurement helper: the device's empirical HBM read-stream rate in GB/s — a trivial sum kernel over
 * `bytes` (use >= 4 GiB: far more than the 256 MiB Infinity Cache), best of a few repetitions and of two read forms
 * (grid-stride default-policy loads; one contiguous span per workgroup with non-temporal loads). */
int smafa_hbm_read_probe(int device, uint64_t bytes, double *gb_per_s);

/* ----------------------------------------------------------------- encoding */
/* Replaces create_lut/BYTE_LUT/encode_single (src/lib.rs:167-196) and the per-byte half of
 * SeqEncodingLength::from_bytes (src/lib.rs:29-52).  On a byte outside the alphabet returns
 * SMAFA_ERR_PANIC and stores its offset in *bad_pos (the reference's panic at src/lib.rs:36-42). */
int smafa_encode(int alphabet, const uint8_t *ascii, uint64_t len, uint8_t *codes, uint64_t *bad_pos);
/* Replaces WindowSet::get_as_string (src/lib.rs:113-135): codes -> "ACGTN" (or the AA letters). */
int smafa_decode(int alphabet, const uint8_t *codes, uint64_t len, char *out);

/* ------------------------------------------------------------ subject store */
/* WindowSet::new (src/lib.rs:63-69) on `device`; seq_len fixes the equal-length invariant of
 * src/lib.rs:91-111 up front (the host checks lengths before it calls append). */
int smafa_db_create(smafa_db **out, int device, int alphabet, uint32_t seq_len);
/* push_encoding x n (src/lib.rs:91-111): packs n rows of code bytes into the HBM bit-plane block.
 * The host buffer is borrowed for the call only. */
int smafa_db_append(smafa_db *db, const uint8_t *codes, uint64_t n);
/* The packed store file: a resident store saved exactly as it lies in HBM — layout tables, bit-plane
 * tiles, subject order, zone words — so that loading it is a memory map and three host-to-device copies instead of the
 * postcard decode of src/lib.rs:208-218 (<= 46 bytes of varints per subject) plus a re-pack.  The file starts with
 * varint(3): the reference rejects it with its own "Unsupported db file version" panic (src/lib.rs:214-217).
 * Written by `smafa makedb --packed`, accepted wherever a DB file is (smafa_query, smafa_dbfile_read). */
int smafa_db_save(smafa_db *db, const char *path);
int smafa_db_load(smafa_db **out, int device, const char *path);
int smafa_db_info(const smafa_db *db, smafa_db_info_t *info);
/* Launch on a caller-owned HIP stream (hipStream_t as void*) instead of the handle's own; NULL restores it. */
int smafa_db_set_stream(smafa_db *db, void *hip_stream);
void smafa_db_destroy(smafa_db *db); /* NULL-safe */

/* ---------------------------------------------------------------- the scan */
/*
 * Replaces WindowSet::get_distances (src/lib.rs:71-89) + the threshold half of the
 * selection in query (src/lib.rs:241-315) / cluster (src/cluster.rs:51-68).
 *
 * Emits every (query, subject, dist) with
 *      dist <= max_div                       (max_div = SMAFA_NONE: no bound)
 *  and dist <= kth(query)                    (max_num_hits = k >= 1: kth = the k-th smallest
 *                                             distance of that query over the whole store, ties
 *                                             included — src/lib.rs:250-256; SMAFA_NONE/0: no bound)
 * ordered by (query, dist, subject) — the reference's print order (src/lib.rs:243-250, 307-311).
 * With k = 1 this is "all subjects at the minimum distance" (src/lib.rs:296-313) and also
 * cluster's argmin with ties to the lowest index (src/cluster.rs:54-68: first row per query).
 * The device may emit rows above kth(query) (its threshold only ever tightens); those are
 * removed before this call returns.
 * cap = capacity of `out` in rows.  If more rows qualify: SMAFA_ERR_CAPACITY, *n_out = rows needed; the handle
 * keeps those rows, and the same call repeated with a larger buffer (same query bytes and bounds, store
 * unchanged) is answered from them without a second scan.  Any other call to smafa_scan_hits drops them.
 */
int smafa_scan_hits(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div,
                    uint32_t max_num_hits, smafa_hit *out, uint64_t cap, uint64_t *n_out);

/* The literal get_distances seam (src/lib.rs:71-89): all N distances of ONE query, as u32.
 * Costs N*4 bytes over PCIe per query — for tests and debugging, not the production path. */
int smafa_distances(smafa_db *db, const uint8_t *query_codes, uint32_t *distances);

/* ---- device-resident batch form (what bench.py times; inputs already in HBM) ---- */
int smafa_qset_create(smafa_qset **out, smafa_db *db, const uint8_t *query_codes, uint64_t n_queries);
void smafa_qset_destroy(smafa_qset *qs);
/*
 * Asynchronous scan of a resident query set against the resident store on the handle's stream.
 * d_hits: device buffer of cap smafa_hit rows (unordered on return); d_count: device uint64 that
 * receives the number of qualifying rows — exact at any capacity with a fixed bound (max_num_hits absent): it may
 * exceed cap, only the first cap rows to arrive are stored, and a caller can size its buffer from it.  In the
 * tightening modes (max_num_hits = k) a value above cap only says "did not fit".  A fixed-bound scan is ONE kernel
 * launch (sets of up to 64 queries: a one-workgroup kernel that zeroes *d_count in front of it); nothing has to be reset between calls.  (The first scan after a store has grown by a quarter through many
 * appends first sorts it again on the device and waits for that — milliseconds, outside the timed kernel.)
 * max_div / max_num_hits as in smafa_scan_hits, except that rows above kth(query) may remain: rows are kept
 * when dist <= the device's final bound of their query, which is exact for k = 1 and >= kth(query) for k >= 2.
 */
int smafa_scan_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, uint32_t max_num_hits, void *d_hits,
                      uint64_t cap, void *d_count);
/* One store pass PER QUERY of a resident set — north_star's literal "each query is broadcast against all subjects" — all
 * enqueued back to back by this one call (no host round trip between passes): query i's rows go to
 * d_hits + i * cap_per_query (rows), its exact count to the i-th uint64 of d_counts (zeroed once for all passes, then each
 * pass reserves its rows from its own counter).  Each pass is the
 * fixed-bound scan smafa_scan_launch runs for a one-query set; with the zone level off (smafa_set_zone_level 0) it
 * streams the prefilter's whole bit-plane: the HBM-bound form bench.py's `stream` leg times.  use_graph != 0: the passes
 * are captured once as a HIP graph and replayed while the arguments stay the same.  Replaces the same loop as
 * smafa_scan_launch (src/lib.rs:232-318 around get_distances, :238), one query per iteration as the reference runs it. */
int smafa_scan_each(smafa_db *db, smafa_qset *qs, uint32_t max_div, void *d_hits, uint64_t cap_per_query, void *d_counts,
                    int use_graph);
int smafa_sync(smafa_db *db);
/* Device time in ms of the scan kernel(s) of the most recent smafa_scan_launch / smafa_scan_hits on
 * this handle, from HIP events recorded on the launch stream; also how many kernel launches it took. */
int smafa_last_scan_ms(smafa_db *db, float *ms, uint32_t *n_launches);
/* Totals over the most recent smafa_scan_hits call on this handle (a best-hit or k-th call without a tight bound is
 * several scans: the near-hit ladder, then the tightening path): device time of the scan kernels, kernel launches, scans. */
int smafa_last_call_stats(smafa_db *db, float *kernel_ms, uint32_t *n_launches, uint32_t *n_scans);
/* Where this handle's scan kernels were really launched: the HIP device that was current on the launching host thread at
 * the most recent launch (-1: none yet), and how many launches of the handle's life were issued while another device than
 * smafa_db_info().device was current (must stay 0).  A multi-device caller — smafa_group_*, smafa_cluster_multi, one host
 * thread per member — checks with this that replica g really runs on devices[g] and not silently on device 0. */
int smafa_launch_device(smafa_db *db, int *device_at_last_launch, uint64_t *launches_off_device);
/* How the most recent scan kernel launch on this handle was laid out: whether it kept only the prefilter's plane
 * of each subject resident (then a sparse-hit scan streams words_per_plane*4 bytes per subject instead of
 * bytes_per_subject), wave tiles per wave, and query blocks (= passes over the store). */
int smafa_last_scan_plan(smafa_db *db, uint32_t *filter_plane_resident, uint32_t *tiles_per_wave, uint32_t *query_blocks);
/* Name of the scan kernel instantiation the most recent launch on this handle used, spelled the way rocprofv3
 * lists it (e.g. "smafa::scan_lazy_kernel<5, 5, 2, 4, false>"), so that a bench line and a profile can be matched. */
int smafa_last_scan_kernel(smafa_db *db, char *name, uint64_t cap);
/* Every distinct kernel instantiation the most recent smafa_scan_hits, smafa_scan_launch, smafa_scan_each or smafa_distances
 * call on this handle launched from the scan family (seed passes, near-hit ladder steps, k-th counting and append passes,
 * index probes), spelled as the demangled template-id ("smafa::scan_kernel<5, 5, 2, 1, false, 1>"), newline-separated
 * in first-launch order and NUL-terminated.  A scan_wide_kernel launch with its zone level on adds the marker line
 * "<template-id> (zone level on)" after the template-id; a kth_seed_kernel launch that counts a whole sample of the store
 * into the per-query counts (not only the seed bound of the first tiles) adds "<template-id> (sample counts)" in the same
 * way.  SMAFA_ERR_CAPACITY if the list needs more than cap bytes. */
int smafa_last_call_kernels(smafa_db *db, char *names, uint64_t cap);
/* Tuning knob: queries per workgroup pass (0 = automatic). */
int smafa_set_query_block(smafa_db *db, uint32_t queries_per_block);
/* 1 (default): the scan evaluates an exact lower bound first and runs the full comparison only where it can
 * still qualify; 0: every (query, subject) pair gets the full comparison.  Results are identical either way. */
int smafa_set_prefilter(smafa_db *db, int enabled);
/* The zone level of a sorted store (scan_zone_kernel: a lower bound on the distances of all 256 subjects of a wave tile
 * at once, from the filter bits they share): 1 (default) = where the store's sorted runs make it prune, 0 = never (every
 * pass streams the prefilter's plane: the HBM-bound form), 2 = whenever the filter-plane-resident kernel runs.  Results
 * are identical in every mode. */
int smafa_set_zone_level(smafa_db *db, int mode);
/* The block index of a resident store — for callers that scan the same store many times with a tight fixed bound (a service,
 * `smafa cluster`'s batches).  The L columns are cut into max_divergence + 1 disjoint blocks; a subject within d <= max_divergence
 * of a query agrees with it on every column of at least one of any d + 1 blocks (it has at most d mismatching columns), so a
 * fixed-bound scan probes d + 1 blocks per query in per-block sorted key arrays and compares in full only the subjects that
 * share a block with the query: the rows of get_distances (src/lib.rs:71-89) + the bound test of :252/:299 without visiting
 * the other subjects.  Exact — the rows are those of the scan kernels, in the same unordered list.  smafa_scan_launch /
 * smafa_scan_hits / the group and session calls use it by themselves when it is current (no append, re-sort or re-plane since
 * it was built), the bound is within it, the batch has more than 64 queries and the store's blocks are selective enough
 * (smafa_index_info().max_div_served; dense families and low-complexity columns are left to the scan kernels); otherwise
 * they scan as before.  Costs 8 bytes x blocks per subject of HBM and about a millisecond per block and 10M subjects to build.
 * Rows of up to 128 columns. */
int smafa_db_build_index(smafa_db *db, uint32_t max_divergence);
int smafa_db_drop_index(smafa_db *db);
int smafa_index_info(const smafa_db *db, smafa_index_info_t *info);
/* 0: a built index is never used; 1 (default): used where it pays; 2: also BUILT by the first big fixed-bound scan that could
 * use one (a synchronous build inside that call); 3: built once the scans that could have used one have cost as much kernel
 * time as the build would (rent or buy: at most twice the best choice in hindsight).  Results are identical in every mode. */
int smafa_set_index(smafa_db *db, int mode);

/* ---------------------------------------------------------------- the self-join */
/*
 * "Which of the store's own rows are near each other": every unordered pair {i, j}, i != j, of the store's subjects with
 * distance <= max_div, exactly once, as smafa_hit{query = min(i, j), subject = max(i, j), dist} (subject numbers = append
 * order, as everywhere else).  Not in the reference; the neighbour list behind dereplication and single-linkage clustering.
 * Rows never visit the host: blocks of the sorted store's own bit-planes become query records on the device, each block is
 * scanned with the fixed-bound kernels of smafa_scan_launch against the part of the store from the block's span onwards only,
 * and a filter pass keeps each pair once.  (Only where 64 rows alone have more rows within the bound than the join's scratch
 * list may hold — millions of near-identical subjects — the call fails: SMAFA_ERR_NOMEM, the count in smafa_last_error(); the handle stays usable.)  Equal rows (distance 0) are pairs like any other; an empty or one-row store gives
 * none; max_div >= seq_len gives all n(n-1)/2 pairs; max_div = SMAFA_NONE is SMAFA_ERR_INVALID.
 * smafa_set_prefilter / smafa_set_zone_level / smafa_set_index keep their meaning (a current block index answers the
 * blocks, modes 2 / 3 may build one on the way); the rows are the same under every setting.
 *
 * smafa_db_self_launch: device-resident form.  d_hits = device buffer of cap rows, unordered on return; *d_count (device
 * uint64) = the exact number of qualifying pairs at ANY capacity — only the first cap rows to arrive are stored; cap = 0 with
 * d_hits = NULL counts only.  The call synchronises the handle's stream between its blocks (it sizes its scratch list from
 * each block's row count) and once at its end; smafa_sync is still the documented way to wait for the results.
 * smafa_last_scan_ms / smafa_last_call_stats then hold the device time and launches of all its blocks (record building,
 * scans and filter passes), smafa_last_call_kernels the scan-family instantiations it launched followed by the join's own
 * kernels (smafa_join::...).
 *
 * smafa_db_self_hits: host form, rows ordered by (query, dist, subject).  cap = capacity of `out` in rows; if more pairs
 * qualify: SMAFA_ERR_CAPACITY, *n_out = rows needed — grow and retry.  Nothing is kept for the retry: it scans again.
 */
int smafa_db_self_launch(smafa_db *db, uint32_t max_div, void *d_hits, uint64_t cap, void *d_count);
int smafa_db_self_hits(smafa_db *db, uint32_t max_div, smafa_hit *out, uint64_t cap, uint64_t *n_out);

/* ------------------------------------------------- single-linkage components of the store */
/*
 * "Which of the store's rows belong together at bound max_div": the graph whose vertices are the store's subjects (numbered in
 * append order) and whose edges are the pairs at distance <= max_div — the self-join's pairs — and per subject i
 * labels[i] = the SMALLEST subject number in i's connected component.  So labels[i] <= i, labels[labels[i]] == labels[i], the
 * rows with labels[i] == i are the representatives (the first-appended member of each component) and *n_components is their
 * number.  Not in the reference (`smafa cluster` is greedy and order-dependent; this is transitive and canonical).  The
 * labels are fully determined by the store and max_div: the same bytes under smafa_set_prefilter / smafa_set_zone_level /
 * smafa_set_index and every SMAFA_JOIN_* setting.
 * The pairs never leave the device and are never listed for the caller: the self-join's blocks are scanned as for
 * smafa_db_self_launch, and each block's scratch list is consumed in place by a concurrent union-find over one uint32 per
 * subject (handle-owned scratch, 4 B per subject), the larger root hooked under the smaller; a last pass writes the labels.
 * Output is n_subjects labels, however many pairs there are.  No filter pass and no inverse order map run.
 * Equal rows (distance 0) are joined at any bound; an empty store gives 0 components and writes no label; one row gives
 * labels = {0}, 1 component; max_div >= seq_len gives all zeros and 1 component (n >= 1; nothing is scanned);
 * max_div = SMAFA_NONE is SMAFA_ERR_INVALID.  A NULL handle, labels or count is SMAFA_ERR_INVALID, and smafa_last_error()
 * names the argument.  The self-join's one failure is inherited unchanged: where 64 rows alone have more rows within the
 * bound than the scratch list may hold, SMAFA_ERR_NOMEM, and the handle stays usable.
 *
 * smafa_db_self_components_launch: device-resident form.  d_labels = device buffer of n_subjects uint32 (smafa_db_info),
 * *d_n_components = device uint64.  Synchronisation as for smafa_db_self_launch: the call synchronises the handle's stream
 * between its blocks and at its end; smafa_sync is still the documented way to wait for the results.
 * smafa_last_scan_ms / smafa_last_call_stats then hold the device time and launches of record building, scans, link
 * passes and the flatten pass; smafa_last_call_kernels lists the scan-family instantiations first, then
 * smafa_join::store_records_kernel, then the smafa_cc:: kernels that ran.
 *
 * smafa_db_self_components: host form.  cap = capacity of `labels` in entries; cap < n_subjects is SMAFA_ERR_INVALID (the
 * caller knows n_subjects from smafa_db_info; there is nothing to grow and retry).
 */
/* device form: d_labels = device buffer of n_subjects uint32; d_n_components = device uint64 */
int smafa_db_self_components_launch(smafa_db *db, uint32_t max_div, void *d_labels, void *d_n_components);
/* host form: cap = capacity of labels in entries, must be >= n_subjects */
int smafa_db_self_components(smafa_db *db, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components);

/* ------------------------------------------------- single-linkage levels: the components at every bound 0 .. max_div */
/*
 * "At which bound do the store's rows belong together": the partitions of smafa_db_self_components at EVERY bound
 * t = 0, 1, .. max_div, from one self-join.  labels is level-major, (max_div + 1) x n_subjects uint32:
 * labels[t * n_subjects + i] = the smallest subject number in i's component of the graph whose edges are the pairs at
 * distance <= t.  Row t is, byte for byte, what smafa_db_self_components(db, t) writes, and n_components[t]
 * (max_div + 1 uint64) is what it counts.  The rows nest: labels[t+1][i] <= labels[t][i],
 * labels[t+1][labels[t][i]] == labels[t+1][i], and the counts never increase with t.  Not in the reference.
 * The join at the largest bound lists every pair within it together with its distance, so the partitions at the smaller
 * bounds are in the same rows: the store is joined ONCE, at bound min(max_div, seq_len - 1), and each piece's scratch
 * list is consumed in place by one union-find per scanned level (handle-owned scratch, 4 B x n_subjects x
 * (min(max_div, seq_len - 1) + 1)); a row at distance d is united at every level from d upwards.  Levels t >= seq_len are
 * all zeros with 1 component and are written without a scan.  The pairs never leave the device.
 * The answer is a function of the store and max_div alone: the same bytes under smafa_set_prefilter /
 * smafa_set_zone_level / smafa_set_index and every SMAFA_JOIN_* setting.
 * An empty store writes no label and counts of 0; one row gives labels all 0 and counts all 1; max_div = SMAFA_NONE, a NULL
 * handle, NULL labels or a NULL count is SMAFA_ERR_INVALID, and smafa_last_error() names the argument.  The self-join's one
 * failure is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list; the handle stays usable),
 * and a failed allocation of the levelled scratch is an error code like any other allocation of the handle's.
 *
 * smafa_db_self_levels_launch: device-resident form.  d_labels = device buffer of (max_div + 1) x n_subjects uint32,
 * d_n_components = device buffer of max_div + 1 uint64.  Synchronisation as for smafa_db_self_components_launch.
 * smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of record building, scans, link passes
 * (the initialisation included) and the flatten pass; smafa_last_call_kernels lists the scan-family instantiations first,
 * then smafa_join::store_records_kernel, then the smafa_lv:: kernels that ran.  No smafa_cc:: kernel is launched.
 *
 * smafa_db_self_levels: host form.  cap = capacity of `labels` in entries; cap < (max_div + 1) * n_subjects is
 * SMAFA_ERR_INVALID.  n_components holds max_div + 1 entries.
 */
int smafa_db_self_levels_launch(smafa_db *db, uint32_t max_div, void *d_labels, void *d_n_components);
int smafa_db_self_levels(smafa_db *db, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components);

/* ------------------------------------------------- minimum spanning forest: the merge tree of single linkage */
/*
 * "Which pair joined them, and at which bound": smafa_db_self_levels says which rows belong together at every bound
 * t = 0 .. max_div, as (max_div + 1) x n_subjects labels; this call gives the same hierarchy as the TREE behind it, at most
 * n_subjects - 1 edges of 12 bytes: what a dendrogram, a cut at a height chosen afterwards or a linkage matrix is made from.
 * The graph is the one of smafa_db_self_components — vertices the store's subjects, edges the pairs within max_div — with an
 * edge's weight its distance, and the result is a minimum spanning forest of it:
 *   edges       smafa_hit{query = a, subject = b, dist}, a < b, dist = the true distance of subjects a and b, ordered by dist
 *               ascending;
 *   level_ends  max_div + 1 uint64: level_ends[t] = the number of edges with dist <= t.
 * For every t the edges [0, level_ends[t]) are acyclic and their connected components are exactly the components of
 * smafa_db_self_components(db, t); hence level_ends[t] = n_subjects - n_components[t], and level_ends[max_div] is the number
 * of edges written.  WHICH of several edges of equal weight is chosen is not fixed and may differ from run to run and
 * between settings; the number of edges per level and the partitions after every level are functions of the store alone,
 * the same under smafa_set_prefilter / smafa_set_zone_level / smafa_set_index and every SMAFA_JOIN_* setting.  Not in the
 * reference.
 * The store is joined ONCE, at bound min(max_div, seq_len - 1); the join only moves its pairs, each once, to a handle-owned
 * list on the device (12 B per pair, at most SMAFA_DENSITY_KEEP_MAX rows — the list and the knob of smafa_db_self_density).
 * Kruskal's algorithm then runs by weight class on the device: one launch per distance 0, 1, .. over that list, a concurrent
 * union-find (4 B per subject) in which the lane whose own compare-and-swap hooked two sets together writes the edge.  Where
 * the pairs exceed the list, the store is instead joined once more per class, at the bounds 0, 1, ..: the same forest
 * property at the cost of those joins.  The pairs never leave the device.
 * Bounds no two rows can exceed (max_div >= seq_len): the components call says "one component" there, and the forest is a
 * spanning tree — after the level seq_len - 1 every remaining component's smallest subject r != 0 gets the edge
 * (0, r, seq_len), whose distance is exactly seq_len, and level_ends[t] = n_subjects - 1 for t >= seq_len.  Nothing is
 * scanned above seq_len - 1.
 * An empty store or one row gives no edge and level_ends all 0 (nothing is scanned); max_div = SMAFA_NONE, a NULL handle,
 * NULL edges or NULL level_ends is SMAFA_ERR_INVALID, and smafa_last_error() names the argument.  The self-join's one failure
 * is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list; the handle stays usable); a partial
 * list is never spanned.
 *
 * smafa_db_self_forest_launch: device-resident form.  d_edges = device buffer of n_subjects - 1 smafa_hit (fewer are
 * written where the forest has several trees; the edges inside a level are in no particular order), d_level_ends = device
 * buffer of max_div + 1 uint64.  Synchronisation as for smafa_db_self_components_launch.  smafa_last_scan_ms /
 * smafa_last_call_stats hold the device time and launches of record building, scans, keep passes, the span launches and the
 * star launch; smafa_last_call_kernels lists the scan-family instantiations first, then smafa_join::store_records_kernel and
 * smafa_join::inverse_order_kernel where it ran, then the smafa_sf:: kernels that ran.  No smafa_cc::, smafa_lv:: or
 * smafa_dn:: kernel is launched.
 *
 * smafa_db_self_forest: host form.  cap = capacity of `edges` in rows; cap < n_subjects - 1 is SMAFA_ERR_INVALID and nothing
 * is written.  The edges of one level are additionally ordered by (query, subject), so a given forest prints one way;
 * level_ends holds max_div + 1 entries.
 */
int smafa_db_self_forest_launch(smafa_db *db, uint32_t max_div, void *d_edges /* n_subjects - 1 smafa_hit */, void *d_level_ends /* max_div + 1 uint64 */);
int smafa_db_self_forest(smafa_db *db, uint32_t max_div, smafa_hit *edges, uint64_t cap, uint64_t *level_ends);

/* ------------------------------------------------- mutual-reachability forest: the merge tree of the density clusters */
/*
 * "The density clusters at EVERY bound, for one min_pts": smafa_db_self_density cures single linkage's chaining at one bound
 * per call, smafa_db_self_forest gives every bound from one join but chains.  This call gives the hierarchy HDBSCAN starts
 * from: a minimum spanning forest under the mutual-reachability distance.  Subjects are numbered in append order;
 * D = max_div, M = min_pts (0 is taken as 1, as in the density call), L = seq_len, n = n_subjects.
 *   ball(i, t)  = 1 + the number of OTHER subjects j != i with distance(i, j) <= t.  The row counts itself, and equal rows at
 *                 different numbers count, exactly as smafa_db_self_density counts (degree[i] + 1 at bound t).
 *   core[i]     = the smallest t in 0 .. D with ball(i, t) >= M; SMAFA_NONE if there is none: the row is SPARSE at D.  M <= 1
 *                 gives core 0 everywhere, M = 2 the nearest-neighbour distance; in general it is the distance to the
 *                 (M - 1)-th nearest other row, entry M - 2 of the row's list from smafa_db_self_neighbours(max_num_hits =
 *                 M - 1) where that list has M - 1 entries.
 *   the graph     vertices the subjects, edges the pairs (a, b) with distance <= D whose ends are both not sparse, an edge's
 *                 weight w = max(distance(a, b), core[a], core[b]), so 0 <= w <= D.
 *   edges       smafa_hit{query = a, subject = b, dist = w}, a < b, ordered by w ascending;
 *   level_ends  max_div + 1 uint64: level_ends[t] = the number of edges with w <= t;
 *   cores       n_subjects uint32, optional: core[i].
 * For every t the edges [0, level_ends[t]) are acyclic and their connected components are exactly the components of the
 * graph cut at weight t.  A pair has w <= t iff it is within t and both ends are core at t, so restricted to the rows with
 * core <= t these components are byte for byte the core-row labels of smafa_db_self_density(db, t, M); rows with core > t are
 * singletons; level_ends[t] = n_subjects minus the number of sets.  WHICH of several pairs of equal weight is chosen is free
 * and may differ from run to run; cores, the counts per level and the partitions are functions of the store, D and M alone,
 * the same under smafa_set_prefilter / smafa_set_zone_level / smafa_set_index, every SMAFA_JOIN_* setting and
 * SMAFA_DENSITY_KEEP_MAX.  M <= 1: the result satisfies the contract of smafa_db_self_forest as it stands (w is the distance).
 * Not in the reference.
 * The store is joined ONCE, at bound min(D, L - 1); the join moves its pairs, each once, to the kept list of
 * smafa_db_self_forest and tallies every pair at both ends, per distance (4 B x (min(D, L - 1) + 1) per subject, handle-owned,
 * exact at any capacity of the list).  The cores come from the tallies, and Kruskal's algorithm then runs by weight class as
 * for the plain forest, a pair weighed by its ends' cores.  Where the pairs exceed the list, the store is joined once more
 * per class t at bound t: every pair of weight t is within t.
 * Bounds no two rows can exceed (D >= L): nothing is scanned above L - 1.  If n >= M, every row still sparse after class
 * L - 1 has core exactly L (every other row is within L), every surviving root r != 0 gets the edge (0, r, L) — two rows in
 * different sets after class L - 1 are either L apart or have an end of core L — and level_ends[t] = n - 1 for t >= L.  If
 * n < M every row is sparse, there is no edge and level_ends is all 0.
 * n = 0 or 1: no scan and no edge, level_ends all 0, cores 0 where M <= 1, else SMAFA_NONE.  max_div = SMAFA_NONE, a NULL
 * handle, NULL edges or NULL level_ends is SMAFA_ERR_INVALID, smafa_last_error() names the argument, and nothing is written.
 * The self-join's SMAFA_ERR_NOMEM is inherited unchanged; a partial list is never spanned.
 *
 * smafa_db_self_reach_forest_launch: device-resident form.  d_edges = device buffer of n_subjects - 1 smafa_hit (the edges
 * inside a level are in no particular order), d_level_ends = device buffer of max_div + 1 uint64, d_cores = device buffer of
 * n_subjects uint32, or NULL.  Synchronisation as for smafa_db_self_components_launch.  smafa_last_call_kernels lists the
 * scan-family instantiations first, then smafa_join::store_records_kernel, smafa_join::inverse_order_kernel where it ran,
 * smafa_sf::init_forest_kernel, smafa_mr::tally_keep_kernel, smafa_mr::core_dist_kernel, smafa_mr::span_reach_kernel where it
 * ran and smafa_sf::star_roots_kernel where it ran.
 *
 * smafa_db_self_reach_forest: host form.  cap = capacity of `edges` in rows; cap < n_subjects - 1 is SMAFA_ERR_INVALID and
 * nothing is written.  The edges of one level are additionally ordered by (query, subject); level_ends holds max_div + 1
 * entries, cores n_subjects entries or is NULL.
 */
int smafa_db_self_reach_forest_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_edges /* n_subjects - 1 smafa_hit */, void *d_level_ends /* max_div + 1 uint64 */, void *d_cores /* n_subjects uint32, may be NULL */);
int smafa_db_self_reach_forest(smafa_db *db, uint32_t max_div, uint32_t min_pts, smafa_hit *edges, uint64_t cap, uint64_t *level_ends, uint32_t *cores /* n_subjects entries, may be NULL */);

/* ------------------------------------------------- stable clusters: HDBSCAN's selection over the mutual-reachability forest */
/*
 * "One label per subject, chosen per region of the data at the level where that region's cluster is most persistent": the
 * step behind smafa_db_self_reach_forest.  Distances here are integers 0 .. D, ties are the rule, so the textbook's binary
 * merges and lambda = 1 / distance are ill-defined; this is the LEVEL-WISE definition, an exact integer function of the store
 * and of D = max_div, M = min_pts (0 is taken as 1) and S = min_cluster_size (0 is taken as max(M, 1)) alone.
 *   levels      core[] is the reach forest's.  For t in 0 .. D, lab_t[i] = the smallest subject number of subject i's set in
 *               that call's graph cut at weight t (the partitions its level_ends delimit, with its rules for D >= L and n < M).
 *               Subject i is IN at t iff core[i] <= t.  size_t(r) = the number of subjects in at t with lab_t[i] == r; a subject
 *               that is not in is a singleton of size 0.  A component (t, r) is BIG iff size_t(r) >= S.  kids(t, r) = the
 *               number of big components (t - 1, r') with lab_t[r'] == r; kids(0, .) = 0.
 *   clusters    A big component STARTS a cluster iff kids != 1; otherwise it CONTINUES the cluster of its one big child.  A
 *               cluster C is therefore a chain of components (t_lo, r_lo) .. (t_hi, r_hi).  Its parent is the cluster started
 *               at (t_hi + 1, lab_{t_hi + 1}[r_hi]) when t_hi < D (that component has kids >= 2); when t_hi == D it is a root.
 *               stability(C) = the sum over t = t_lo .. t_hi of size_t(r_t), as uint64.  This is HDBSCAN's
 *               sum over points (lambda_p - lambda_birth) with lambda measured in LEVELS instead of 1 / distance; the
 *               result depends on D through the roots' lifetime: a larger D lengthens every root and nothing else.
 *   selection   (excess of mass)  best(C) = max(stability(C), the sum of best(child) over C's children).  C is CHOSEN iff
 *               stability(C) >= that sum (a leaf's sum is 0; a tie goes to the parent) and no ancestor of C is chosen.
 *   labels      n_subjects uint32: labels[i] = r_hi of the chosen cluster C with core[i] <= t_hi and lab_{t_hi}[i] == r_hi —
 *               there is at most one —, SMAFA_NONE where there is none: noise.  A label is the smallest subject number of its
 *               cluster.
 *   joined      n_subjects uint32, optional: the smallest t in [t_lo, t_hi] at which subject i is in and in C's component;
 *               the subjects of C's descendant clusters get t_lo; noise gets SMAFA_NONE.
 *   n_clusters  one uint64 ON THE HOST in both forms: the number of chosen clusters.
 *   cores       n_subjects uint32, optional: core[i], as smafa_db_self_reach_forest gives it.
 * Every output is the same from run to run and under smafa_set_prefilter / smafa_set_zone_level / smafa_set_index, every
 * SMAFA_JOIN_* setting and SMAFA_DENSITY_KEEP_MAX.  Not in the reference.
 * The call runs smafa_db_self_reach_forest_launch's passes into handle-owned buffers and then works from the at most n - 1
 * edges and the cores alone: the edges are united class by class over a fresh union-find, and behind every class the root,
 * the size and the big children of every component are recorded; the selection runs once up and once down the levels.  Levels
 * above L are never scanned, allocated or launched: they are all alike, and their share of a stability, size x (D - L + 1), is
 * added arithmetically.  The number of launches behind the forest is 5 x (min(D, L) + 1) + 2 whatever the store holds.  HBM
 * on top of the reach forest's: 4 B x 2 x (min(D, L) + 1) per subject for the root and flag planes, 44 B per subject of
 * per-level state, 12 B per subject for the edges and 8 B x (D + 1).
 * n = 0: nothing is written but *n_clusters = 0.  n = 1: no scan; with M <= 1 and S <= 1 the subject is one cluster, label 0,
 * joined 0; otherwise noise; cores as the reach forest's.
 * Argument checks, in this order, each SMAFA_ERR_INVALID with smafa_last_error() naming the argument and NOTHING written: a
 * NULL handle; NULL labels; NULL n_clusters; max_div == SMAFA_NONE; host form only: cap < n_subjects.  The self-join's
 * SMAFA_ERR_NOMEM is inherited unchanged.
 *
 * smafa_db_self_stable_launch: device-resident form.  d_labels, d_joined (or NULL), d_cores (or NULL) = device buffers of
 * n_subjects uint32.  The call waits for its own work — *n_clusters is valid on return, and so are the buffers.
 * smafa_last_call_kernels lists the reach forest's kernels as that call lists them, then smafa_st::unite_class_kernel,
 * smafa_st::snapshot_kernel, smafa_st::census_kernel (more than one level), smafa_st::adopt_kernel, smafa_st::excess_kernel,
 * smafa_st::choose_kernel and smafa_st::assign_kernel.
 *
 * smafa_db_self_stable: host form.  cap = capacity of `labels` — and of `joined` and `cores` where given — in entries.
 */
int smafa_db_self_stable_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, void *d_labels /* n_subjects uint32 */, void *d_joined /* n_subjects uint32, may be NULL */, void *d_cores /* n_subjects uint32, may be NULL */, uint64_t *n_clusters /* host */);
int smafa_db_self_stable(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, uint32_t *labels, uint32_t *joined /* may be NULL */, uint32_t *cores /* may be NULL */, uint64_t cap, uint64_t *n_clusters);

/* ------------------------------------------------- density clusters of the store (DBSCAN over the self-join) */
/*
 * "Which of the store's rows belong together at bound max_div, where enough rows agree": single linkage chains — one sparse
 * run of rows, each one substitution from the next, fuses two abundant families into one component.  Here a row may extend
 * a cluster only if enough rows lie within the bound of it: DBSCAN with eps = max_div over the scan's distance.  Subjects
 * are numbered in append order; min_pts >= 1, and 0 is taken as 1.
 *   degree[i]  = the number of OTHER subjects j != i with distance(i, j) <= max_div.  Equal rows at different subject
 *                numbers count: abundance counts.
 *   core       i is a core row iff degree[i] + 1 >= min_pts (the row counts itself, as in the textbook and in
 *                scikit-learn's min_samples).
 *   clusters   the connected components of the graph on the CORE rows whose edges are the core-core pairs within the bound.
 *                A cluster's label is the smallest CORE subject number in it.
 *   border     a non-core row with at least one core row within the bound.  Its label is the label of its
 *                smallest-NUMBERED core neighbour (textbook DBSCAN leaves this to the visiting order; here it is canonical).
 *   noise      every other row: label SMAFA_NONE.
 *   counts[3]  = {clusters, core rows, noise rows}.
 * The answer is a function of the store, max_div and min_pts alone: the same bytes under smafa_set_prefilter /
 * smafa_set_zone_level / smafa_set_index, every SMAFA_JOIN_* setting and SMAFA_DENSITY_KEEP_MAX.
 * labels[i] <= i holds for CORE rows only: a border row may be numbered below its cluster's label (the label is a core row,
 * the border row is not).  For core rows labels[labels[i]] == labels[i]; every label that is not SMAFA_NONE is a core row.
 *   min_pts <= 1: every row is core, and the labels are byte for byte those of smafa_db_self_components(db, max_div),
 *                 counts = {its n_components, n_subjects, 0}.
 *   min_pts == 2: the clusters are the components of size >= 2, and the singletons are noise.
 * Not in the reference.  The pairs never leave the device.  The self-join's pieces are scanned as for smafa_db_self_launch and
 * each piece's scratch list is consumed in place, in two phases with a kernel boundary between them (whether a row is core
 * is known only once every pair is counted): phase 1 applies the self-join's exactly-once rule to the list, raises both
 * degrees of every kept pair and moves the pair to a handle-owned KEPT PAIR LIST; phase 2 unites core-core pairs in a
 * union-find over the core rows and offers every non-core end of a pair its core neighbour's number (an atomic minimum).
 * Where the kept list held every pair, phase 2 is ONE launch over it and the store is joined once; otherwise the store is
 * joined a second time and phase 2 reads the raw lists.  Both give the same bytes.  SMAFA_DENSITY_KEEP_MAX (environment, read
 * when the handle is made, like SMAFA_JOIN_BLOCK) is the kept list's capacity in rows of 12 B, grown on demand; its default is
 * the value of the join's scratch ceiling (SMAFA_JOIN_SCRATCH_MAX, 2^27 rows); 0 forces the two-join path.  (The list and
 * its capacity are shared with smafa_db_self_peaks below: one list per handle, whichever call fills it.)  Degrees are exact at
 * any capacity.  With no core row at all phase 2 is skipped; with min_pts <= 1 and degrees == NULL nothing needs counting and
 * the one join links directly, as the components call does.  Handle-owned scratch: 4 B x 3 per subject plus the kept list.
 * Edges: an empty store writes nothing and counts 0 / 0 / 0.  max_div >= seq_len: no scan, every degree is n_subjects - 1, and
 * all labels are 0 if n_subjects >= min_pts, otherwise all noise.  min_pts > n_subjects: all noise.  max_div = SMAFA_NONE, or
 * a NULL handle, labels or counts: SMAFA_ERR_INVALID, with the argument named in smafa_last_error().  The self-join's one
 * failure is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list; the handle stays usable).
 *
 * smafa_db_self_density_launch: device-resident form.  d_labels = device buffer of n_subjects uint32, d_degrees = device
 * buffer of n_subjects uint32 or NULL, d_counts = device buffer of 3 uint64.  Synchronisation as for
 * smafa_db_self_components_launch.  smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of record
 * building, scans (of both joins, where two ran), count/keep passes, link passes and the flatten pass;
 * smafa_last_call_kernels lists the scan-family instantiations first, then smafa_join::store_records_kernel, then
 * smafa_join::inverse_order_kernel if it ran, then the smafa_dn:: kernels that ran.
 *
 * smafa_db_self_density: host form.  cap = capacity of `labels` (and of `degrees`, unless NULL) in entries; cap < n_subjects is
 * SMAFA_ERR_INVALID, and nothing is written.
 */
int smafa_db_self_density_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_labels, void *d_degrees /* may be NULL */, void *d_counts /* 3 x uint64 */);
int smafa_db_self_density(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t *labels, uint32_t *degrees /* may be NULL */, uint64_t cap, uint64_t counts[3]);

/* ------------------------------------------------- abundance-peak clusters of the store (amplicon denoising over the self-join) */
/*
 * "Which more abundant row does each row most plausibly derive from": density clusters cure chaining only where the bridge
 * is sparse, and need a threshold.  Where abundance falls off continuously between two abundant rows, every min_pts either
 * fuses them or drops the thin part as noise.  Here every row climbs to the heaviest row within the bound, and a cluster is
 * everything that climbs to the same local maximum (the UNOISE / swarm partition), with no threshold at all.
 * max_div = D is the neighbourhood, radius = r <= D the ball the weight is counted in; radius = SMAFA_NONE means r = D.
 *   weight[i]  = 1 + the number of OTHER subjects within distance r of i.  r = 0 is abundance: the number of exact copies,
 *                itself included.  r = D is the ball count: smafa_db_self_density's degree[i] + 1.
 *   key(i)     = the pair (weight[i], -i) in lexicographic order: the heavier row wins, ties go to the smaller subject number.
 *                It is a total order with no equal keys.
 *   parent[i]  = the subject with the greatest key among {i} and {j : distance(i, j) <= D}.  parent[i] == i makes i a PEAK:
 *                no row within the bound outranks it.
 *   labels[i]  = the peak reached from i by following parent[].  The key strictly increases along every step, so parent[]
 *                is a forest and the walk ends.
 *   n_peaks    = the number of peaks = the number of clusters.
 * The answer is a function of the store, D and r alone: the same bytes under smafa_set_prefilter / smafa_set_zone_level /
 * smafa_set_index, every SMAFA_JOIN_* setting and SMAFA_DENSITY_KEEP_MAX.  Exact copies of one sequence have the same
 * neighbourhood, so all of them get the same parent: the smallest-numbered copy, or the same heavier neighbour.  labels[i]
 * need not be <= i.  labels[labels[i]] == labels[i], and labels[i] lies in i's single-linkage component at D.
 * Not in the reference.  The pairs never leave the device.  Two phases with a kernel boundary between them, as for the
 * density call (a key is known only once every pair is weighed): phase 1 applies the self-join's exactly-once rule to each
 * piece's list, raises both weights of every kept pair within r and moves EVERY kept pair to the handle's kept pair list —
 * the one list the density call uses, so SMAFA_DENSITY_KEEP_MAX is the capacity of that one shared list for both calls, 0
 * forcing the two-join path; phase 2 offers the lower-keyed row of every pair the higher key (an atomic maximum on an 8-byte
 * slot per subject), in ONE launch over the kept list where that held every pair, otherwise in a second join that reads the
 * raw lists.  Both give the same bytes.  With no pair at all phase 2 is skipped.  The labels are then flattened by pointer
 * doubling in place, one launch per round until a round changes nothing (at most 33 rounds; no thread ever walks a chain).
 * Handle-owned scratch: 12 B per subject plus the kept list.
 * Edges: an empty store writes nothing and n_peaks = 0.  One row: labels {0}, parents {0}, weights {1}, 1 peak, no scan.
 * max_div >= seq_len: every row is every row's neighbour, so there is one peak, the row of greatest key, and every parent
 * and label is that row; the weights come from a count-only join at r (nothing is kept, nothing is climbed), and if r >=
 * seq_len too there is no scan at all and every weight is n_subjects.  SMAFA_ERR_INVALID, with the argument named in
 * smafa_last_error() and nothing written: a NULL handle, labels or n_peaks; max_div = SMAFA_NONE; radius > max_div (other
 * than SMAFA_NONE); cap < n_subjects.  The self-join's one failure is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone
 * overfill the scratch list; the handle stays usable).
 *
 * smafa_db_self_peaks_launch: device-resident form.  d_labels = device buffer of n_subjects uint32, d_parents and d_weights =
 * device buffers of n_subjects uint32 or NULL, d_n_peaks = device uint64.  Synchronisation as for
 * smafa_db_self_components_launch.  smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of record
 * building, scans (of both joins, where two ran), weigh/keep passes, the climb, the settle pass and the jump rounds;
 * smafa_last_call_kernels lists the scan-family instantiations first, then smafa_join::store_records_kernel, then
 * smafa_join::inverse_order_kernel if it ran, then the smafa_pk:: kernels that ran: init_peaks_kernel, weigh_keep_kernel,
 * climb_kernel, crown_kernel, settle_kernel, jump_kernel.
 *
 * smafa_db_self_peaks: host form.  cap = capacity of `labels` (and of `parents` and `weights`, unless NULL) in entries.
 */
int smafa_db_self_peaks_launch(smafa_db *db, uint32_t max_div, uint32_t radius, void *d_labels, void *d_parents /* may be NULL */, void *d_weights /* may be NULL */, void *d_n_peaks /* uint64 */);
int smafa_db_self_peaks(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t *labels, uint32_t *parents /* may be NULL */, uint32_t *weights /* may be NULL */, uint64_t cap, uint64_t *n_peaks);

/* ------------------------------------------------- chimera check of the store (two-parent bimeras over the self-join) */
/*
 * "Which rows are one heavier row's head on another heavier row's tail": the step every amplicon denoiser takes behind its
 * partition (UNOISE, UCHIME de novo, DADA2's isBimeraDenovo).  A PCR chimera starts as a copy of one abundant sequence and
 * ends as a copy of another; smafa_db_self_peaks crowns such a row a centre of its own.  For rows of one length, column by
 * column, the check is exact.  Let n = n_subjects, L = seq_len, max_div = D, radius = r <= D (SMAFA_NONE: r = D), min_fold =
 * F >= 1.
 *   weight[i]  exactly as in smafa_db_self_peaks at radius r: 1 + the number of OTHER subjects within r of i.  With weights_in
 *              (n uint32) those are used instead and no weight is counted (r is still checked).  A row of weight 0 takes no
 *              part, neither as a candidate nor as a parent.
 *   p is an ELIGIBLE PARENT of q iff p != q, both weights are non-zero, distance(q, p) <= D (the scan's distance: the number
 *              of columns whose codes differ), weight[p] > weight[q] and (uint64)weight[p] >= (uint64)F * weight[q].
 *   pre(q, p)  for an eligible pair the rows differ in source columns d_0 < ... < d_{m-1}, m >= 1 (copies have equal weights,
 *              so m = 0 never occurs): pre(q, p) = d_0, the length of the common prefix in the CALLER's column order, and
 *              suf(q, p) = L - 1 - d_{m-1}, the length of the common suffix.  (Under weights_in copies may carry unequal weights:
 *              rows that are equal column by column are never each other's parents, whatever their weights.)
 *   left_parent[q]  = the eligible p of greatest (pre(q, p), -p): the longest prefix, ties to the smaller subject number;
 *   left_len[q]     = that prefix length.  right_parent[q], right_len[q]: the same with suf.  Without an eligible parent both
 *              parents are SMAFA_NONE and both lengths 0.
 *   flags[q]   = 1 iff q has an eligible parent and left_len[q] + right_len[q] >= L, else 0.  One parent can never satisfy
 *              this alone: pre + suf = L - 1 - (d_{m-1} - d_0) < L.  A flagged row therefore always has two distinct parents,
 *              and any breakpoint b with L - right_len[q] <= b <= left_len[q] reproduces q as left_parent[:b] + right_parent[b:].
 *   *n_chimeras = the number of flagged rows.
 * Parents are looked for only within D of the candidate.  A bimera's distance to either parent is at most the parents' own
 * distance, so D has to be at least the divergence of the parents one wants to catch.  max_div >= seq_len is legal and means
 * "every other row is a candidate parent": the join then runs at seq_len, as smafa_db_self_hits runs it, and lists every pair —
 * a pair with no column in common has pre = suf = 0 and can change a result only as a parent of last resort at length 0 with
 * the smaller number.  (That is n (n - 1) / 2 pairs: a bound for small stores.)  radius >= seq_len with counted weights gives
 * every row the weight n: no parent anywhere, nothing flagged, no scan.
 * The answer is an exact integer function of the store, D, r, F and weights_in, and the same bytes from run to run and under
 * smafa_set_prefilter / smafa_set_zone_level / smafa_set_index, every SMAFA_JOIN_* setting and SMAFA_DENSITY_KEEP_MAX.
 * The pipeline form: weights_in = the cluster sizes of smafa_db_self_peaks on the peaks and 0 elsewhere checks the centres alone.
 * Not in the reference.  The pairs never leave the device.  Three phases with kernel boundaries between them (chimera.hip.h):
 * phase 1 is the peaks call's — the join at D, each kept pair within r raising both weights and EVERY kept pair moving to the
 * handle's kept pair list (the list of the density and peaks calls: SMAFA_DENSITY_KEEP_MAX is its capacity, 0 forces the
 * two-join path); weights_in is copied over the counted weights behind the join.  Phase 2 takes every pair whose weights make
 * one row an eligible parent of the other, gathers the bit-plane words of both rows, walks the differing packed columns back to
 * source columns and offers (length, -parent) to the lighter row's two 8-byte slots by atomic maximum — in ONE launch over the
 * kept list where that held every pair, otherwise in a second join that reads the raw lists.  Both give the same bytes.  Phase
 * 3 unpacks the slots and counts.  Handle-owned scratch: 20 B per subject plus the kept list.
 * Checks, in this order, each SMAFA_ERR_INVALID with the argument named in smafa_last_error() and nothing written: a NULL
 * handle; NULL flags; NULL n_chimeras; max_div = SMAFA_NONE; radius > max_div (other than SMAFA_NONE); min_fold = 0; host form
 * only: cap < n_subjects.  Then the count is zeroed — the first write — and the arrays are written only by a call that
 * succeeds.  An empty store writes nothing but the count; one row gives flags {0}, both parents SMAFA_NONE, both lengths 0.
 * The self-join's one failure is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list; the
 * handle stays usable).
 *
 * smafa_db_self_chimeras_launch: device-resident form.  d_weights_in = device buffer of n_subjects uint32 or NULL; d_flags and
 * (each or NULL) d_left_parent, d_left_len, d_right_parent, d_right_len, d_weights = device buffers of n_subjects uint32;
 * d_n_chimeras = device uint64.  Synchronisation as for smafa_db_self_peaks_launch.  smafa_last_scan_ms / smafa_last_call_stats
 * hold the device time and launches of record building, scans (of both joins, where two ran), weigh/keep passes, the offers
 * and the verdict; smafa_last_call_kernels lists the scan-family instantiations first, then smafa_join::store_records_kernel,
 * then smafa_join::inverse_order_kernel if it ran, then smafa_pk::init_peaks_kernel, smafa_pk::weigh_keep_kernel (a join ran),
 * chimera::init_sides_kernel, chimera::offer_sides_kernel (a pair was kept) and chimera::verdict_kernel.
 *
 * smafa_db_self_chimeras: host form.  cap = capacity of `flags` (and of the five arrays behind it, unless NULL) in entries.
 */
int smafa_db_self_chimeras_launch(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const void *d_weights_in /* may be NULL */, void *d_flags, void *d_left_parent, void *d_left_len, void *d_right_parent, void *d_right_len, void *d_weights /* the last five may be NULL */, void *d_n_chimeras /* uint64 */);
int smafa_db_self_chimeras(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const uint32_t *weights_in, uint32_t *flags, uint32_t *left_parent, uint32_t *left_len, uint32_t *right_parent, uint32_t *right_len, uint32_t *weights, uint64_t cap, uint64_t *n_chimeras);

/* ------------------------------------------------- neighbour lists of the store (the self-join's graph in CSR form, k nearest) */
/*
 * "Who is near row i, nearest first": the one general output of the self-join, in the form graph tools take (a CSR matrix,
 * community detection, UMAP, HDBSCAN core distances, k-distance plots).  smafa_db_self_hits returns each edge once, under
 * its smaller endpoint; here every row has its own list.  max_div = D is the bound, max_num_hits = k the cut (SMAFA_NONE: no
 * cut).  Subjects are numbered in append order.
 *   N(i)          = { j != i : distance(i, j) <= D }, ordered by (distance, j) ascending.  Exact copies (distance 0) are
 *                   neighbours like any other.
 *   list(i)       = the first min(|N(i)|, k) entries of N(i): ties at the cut go to the smaller subject number.
 *   offsets[i]    = the start of list(i); offsets[n_subjects] = total, the number of entries.  Without a cut
 *                   offsets[i + 1] - offsets[i] is smafa_db_self_density's degree[i] and total is twice the pair count of
 *                   smafa_db_self_launch.
 *   neighbours[], dists[] hold list(i) at offsets[i] .. offsets[i + 1); dists may be NULL.
 * The answer is a function of the store, D and k alone: the same bytes under smafa_set_prefilter / smafa_set_zone_level /
 * smafa_set_index, every SMAFA_JOIN_* setting and SMAFA_NEIGHBOUR_SORT.
 * Capacity as for smafa_db_self_hits: cap = the capacity of `neighbours` (and of `dists`) in entries.  The offsets and the
 * total are exact at any capacity and always written.  total > cap: SMAFA_ERR_CAPACITY, *n_out (*d_total) = the entries
 * needed, neighbours and dists untouched.  cap = 0 with NULL lists asks for the degrees alone.  Nothing is kept for the retry:
 * it joins again.
 * Not in the reference.  The pairs never leave the device: the self-join's exactly-once rule is applied to each piece's list
 * and every kept pair {a, b, d} is appended as two 8-byte entries, (a; d; b) and (b; d; a), to a handle-owned entry list
 * that grows in front of a piece's pass (doubling, live entries carried over).  Behind the join the entries are ordered by
 * (row, dist, neighbour) with the device radix sort — one sort of the entries as keys where row and distance fit 32 bits
 * (the distance field is as wide as min(D, seq_len) needs, the row field as n_subjects - 1 needs), otherwise two stable sorts;
 * SMAFA_NEIGHBOUR_SORT=2, read when the handle is made, forces the latter — a binary search per row finds where each row
 * begins, with a cut the degrees are cut and summed, and one pass over the sorted entries writes the lists.  The host learns
 * the total (with a cut: one wait more) and decides on SMAFA_ERR_CAPACITY.  Handle-owned scratch: 8 (12) B per entry for the
 * list, 8 (24) B per entry for the sort, 16 B per subject with a cut.
 * Edges: an empty store gives offsets {0} and total 0; one row {0, 0}.  max_div >= seq_len is no shortcut — the distances
 * still differ: the join runs at min(max_div, seq_len) and every row lists every other.  SMAFA_ERR_INVALID, with the argument
 * named in smafa_last_error() and nothing written: a NULL handle, offsets or total (n_out); NULL neighbours with a capacity;
 * max_div = SMAFA_NONE; max_num_hits = 0.  More than 2^31 - 1 entries before the cut: SMAFA_ERR_NOMEM with the count in the
 * text (the device sort's item limit); an entry list that cannot grow: SMAFA_ERR_NOMEM; the handle stays usable.  The
 * self-join's own failure is inherited unchanged (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list).
 *
 * smafa_db_self_neighbours_launch: device-resident form.  d_offsets = device buffer of n_subjects + 1 uint64, d_neighbours and
 * d_dists = device buffers of cap uint32 (d_neighbours may be NULL if cap == 0, d_dists may be NULL), d_total = device uint64.
 * Synchronisation as for smafa_db_self_peaks_launch.  smafa_last_scan_ms / smafa_last_call_stats hold the device time and
 * launches of record building, scans, pack passes, the sort, the bounds / cut pass and the emit pass;
 * smafa_last_call_kernels lists the scan-family instantiations first, then smafa_join::store_records_kernel, then
 * smafa_join::inverse_order_kernel if it ran, then the smafa_nb:: kernels that ran: mirror_pack_kernel, row_bounds_kernel,
 * cut_degrees_kernel, emit_kernel (with no entry at all: mirror_pack_kernel alone).
 *
 * smafa_db_self_neighbours: host form.  offsets holds n_subjects + 1 entries.
 */
int smafa_db_self_neighbours_launch(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, void *d_offsets /* n_subjects + 1 uint64 */, void *d_neighbours /* cap uint32, may be NULL if cap == 0 */, void *d_dists /* cap uint32 or NULL */, uint64_t cap, void *d_total /* uint64 */);
int smafa_db_self_neighbours(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, uint64_t *offsets, uint32_t *neighbours, uint32_t *dists /* may be NULL */, uint64_t cap, uint64_t *n_out);

/* ------------------------------------------------- delta self-join: pairs and components of the rows appended since a mark */
/*
 * "I appended m rows; which pairs are new, and what are the components now?" — without joining the whole store again.
 * Subjects are numbered in append order and keep their numbers through every re-sort, so a mark is a subject number:
 * first_row, 0 <= first_row <= n_subjects, and "the new rows" are first_row .. n_subjects - 1.  The work is m x n pair
 * tests, not n x n / 2.
 *
 * Delta pairs (smafa_db_self_since_launch / smafa_db_self_hits_since): every unordered pair {i, j}, i < j, with
 * j >= first_row and distance <= max_div, exactly once, as {query = i, subject = j, dist}.  The pairs of the store's first
 * first_row rows and the delta pairs are disjoint, and together they are the pairs of the whole store.  first_row =
 * n_subjects gives no rows; first_row = 0 the rows of smafa_db_self_hits.  Capacity as for smafa_db_self_hits: the count is
 * exact at any capacity, SMAFA_ERR_CAPACITY names the rows needed, cap = 0 with a NULL list asks for the count alone.  The
 * host form orders its rows by (query, dist, subject); the device form leaves them unordered.
 *
 * Components update (smafa_db_self_components_update_launch / smafa_db_self_components_update): labels[] holds n_subjects
 * entries, in and out.  On entry labels[0 .. first_row) are the labels smafa_db_self_components gave for the store's first
 * first_row rows at the same max_div; the entries from first_row on are ignored.  On return all n_subjects entries and
 * *n_components are byte for byte what smafa_db_self_components(db, max_div) returns on the store as it is now.  What can be
 * checked of the labels given is checked on the device — labels[i] <= i, labels[i] < first_row, labels[labels[i]] ==
 * labels[i] — and a violation is SMAFA_ERR_INVALID with the number of bad entries in smafa_last_error(); labels[] is then
 * untouched and the handle stays usable.  (Labels that pass these checks and still are not the labels of the first rows at
 * this bound give labels of no meaning.)  first_row = 0 is the full call; first_row = n_subjects returns the labels as given
 * and counts their representatives; max_div >= seq_len gives all labels 0.
 *
 * Not in the reference.  The new rows' query records are gathered from the sorted store on the device
 * (smafa_dl::gather_records_kernel, through the position of every subject number), a span of them at a time, and every block
 * of a span is scanned against the whole store by the scan kernels smafa_db_self_launch uses — or answered from a current
 * block index.  The exactly-once rule needs no positions: a row {new row a, partner s} of a block's list is kept iff s < a
 * (smafa_dl::delta_filter_kernel).  The update seeds the union-find of smafa_db_self_components with the labels given
 * (smafa_dl::seed_parents_kernel) and links only the delta join's rows.  Scratch, SMAFA_JOIN_* settings and the one failure of
 * the self-join (SMAFA_ERR_NOMEM where 64 rows alone overfill the scratch list) are those of smafa_db_self_launch.
 * SMAFA_ERR_INVALID, with the argument named in smafa_last_error(): a NULL handle, count or labels; a NULL row buffer with a
 * capacity; max_div = SMAFA_NONE; first_row > n_subjects; cap < n_subjects (update).  Synchronisation of the device forms as
 * for smafa_db_self_launch; d_labels = device buffer of n_subjects uint32, d_count / d_n_components = device uint64.
 * smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of the gather, the scans and the consumer
 * passes; smafa_last_call_kernels lists the scan-family instantiations first, then smafa_dl::gather_records_kernel, then
 * smafa_join::inverse_order_kernel if it ran, then the call's own kernels.
 */
int smafa_db_self_since_launch(smafa_db *db, uint64_t first_row, uint32_t max_div, void *d_hits, uint64_t cap, void *d_count);
int smafa_db_self_hits_since(smafa_db *db, uint64_t first_row, uint32_t max_div, smafa_hit *out, uint64_t cap, uint64_t *n_out);
int smafa_db_self_components_update_launch(smafa_db *db, uint64_t first_row, uint32_t max_div, void *d_labels, void *d_n_components);
int smafa_db_self_components_update(smafa_db *db, uint64_t first_row, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components);

/* ------------------------------------------------- consensus: one sequence per labelled cluster, and the member nearest to it */
/*
 * What each cluster of a label call looks like.  `labels` holds one uint32 per subject, as smafa_db_self_components,
 * _density, _peaks, _stable and the others write them: SMAFA_NONE (the row belongs to no cluster and is left out) or a value
 * below n_subjects.  A value need not be a member's own number.  The call is an exact integer function of the store and the
 * labels and gives the same bytes from run to run.
 *
 * Let r_0 < r_1 < ... < r_{K-1} be the distinct values other than SMAFA_NONE.
 *   ids[k]    = r_k.
 *   sizes[k]  = the number of rows with that label.
 *   codes[k * seq_len + c], for source column c in 0 .. seq_len - 1: the code that the most members of cluster k hold at
 *               column c; a tie goes to the smallest code.  Codes are those of smafa_encode, columns are in the caller's
 *               order, not the store's.  The nucleotide N class (code 4) is a code like any other: it wins a column only with
 *               a strict plurality over every smaller code.
 *   div[i]    (optional, n_subjects uint32) = the scan's distance between row i and codes[k(i)]: the number of columns where
 *               they differ.  SMAFA_NONE for unlabelled rows.
 *   nearest[k] (optional) = the member of cluster k with the smallest (div, subject number).
 *   *n_clusters (host uint64 in both forms) = K.
 *
 * Checks, in this order, each SMAFA_ERR_INVALID with the argument named in smafa_last_error() and nothing written: a NULL
 * handle; NULL labels; NULL n_clusters; NULL ids, sizes or codes while cap_clusters > 0.  Then, from the device: a label that is
 * neither SMAFA_NONE nor below n_subjects gives SMAFA_ERR_INVALID — the text names `labels` and the smallest offending subject
 * number, found with an atomic minimum, so it is the same every run — and nothing is written.  cap_clusters < K gives
 * SMAFA_ERR_CAPACITY with *n_clusters = K and no output array touched: cap_clusters = 0 with NULL arrays is the way to ask for K.
 * An empty store gives *n_clusters = 0 and writes nothing else; all labels SMAFA_NONE gives K = 0 and div all SMAFA_NONE.
 *
 * On the device (consensus.hip.h): the values that occur are marked and numbered by an exclusive sum; the store's positions are
 * sorted by their group's number with one stable radix sort over the bits of K; one wave64 per SMAFA_CONSENSUS_CHUNK sorted
 * entries (read when the handle is made; default 4096, at least 64) reads each plane word of its members once, lanes as
 * columns, counts codes in LDS and votes; a group that crosses such a window adds its counters to one table per window edge,
 * voted by a second small kernel; a last pass measures every row against its group's consensus in bit-plane form and takes the
 * nearest by atomic minimum.  Handle-owned scratch: 16 B per position for the sort, 8 B per subject, 12 + 4 x planes x words B
 * per cluster, 4 KB x words per window — never clusters x columns x alphabet counters.  No other call's state (the inverse order,
 * the kept list, the index) is touched.
 *
 * smafa_db_consensus_launch: device-resident form.  d_labels = n_subjects uint32; d_ids, d_sizes, d_nearest (or NULL) =
 * cap_clusters uint32; d_codes = cap_clusters x seq_len bytes; d_div (or NULL) = n_subjects uint32.  The call waits for its own
 * work, as smafa_db_self_stable_launch does: *n_clusters and the buffers are valid on return.
 * smafa_db_consensus: host form.
 * smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of the call; smafa_last_call_kernels lists
 * consensus::mark_groups_kernel, group_ids_kernel, group_keys_kernel, segment_bounds_kernel, tally_vote_kernel<planes>,
 * vote_tables_kernel<planes> (more than one window), measure_kernel (an optional output asked for) and finish_groups_kernel.
 */
int smafa_db_consensus_launch(smafa_db *db, const void *d_labels, void *d_ids, void *d_sizes, void *d_codes, void *d_nearest /* may be NULL */, void *d_div /* may be NULL */, uint64_t cap_clusters, uint64_t *n_clusters /* host */);
int smafa_db_consensus(smafa_db *db, const uint32_t *labels, uint32_t *ids, uint32_t *sizes, uint8_t *codes, uint32_t *nearest, uint32_t *div, uint64_t cap_clusters, uint64_t *n_clusters);

/* ------------------------------------------------- abundance table: reads assigned to their nearest subject and counted */
/*
 * The last step of an amplicon pipeline: the reads of every sample mapped back to the kept sequences and counted, cluster x
 * sample (`usearch -otutab`, DADA2's sequence table).  Not in the reference.
 * Inputs: the store's n subjects; m reads (a resident query set, or code rows); a bound max_div; per subject a label (uint32, any
 * value; labels NULL: a subject's label is its own number); per read a sample number below n_samples (samples NULL: every read is
 * in sample 0; n_samples >= 1) and a weight (uint32; weights NULL: every read weighs 1 — for dereplicated reads with sizes).
 *   A read is ASSIGNED to the subject at the smallest distance <= max_div, a tie to the smaller subject number (`smafa cluster`'s
 *   argmin rule): subject[q] is that number and dist[q] its distance.  With no subject within the bound, or an empty store, both
 *   are SMAFA_NONE and the read is UNASSIGNED.
 *   A read's label is the label of its subject; an unassigned read has the label SMAFA_NONE — the same "in no cluster" as a noise
 *   label, as in smafa_db_consensus.
 *   The TABLE: one entry {label, sample, count} per (label, sample) that holds at least one read of weight > 0, count the uint64
 *   sum of those reads' weights, ordered by (label, sample) ascending — SMAFA_NONE comes last.
 *   subject_counts[i] (uint64, optional) = the weight of all reads assigned to subject i, over all samples: what
 *   `smafa chimeras --weights` takes.
 *   totals[0] = the number of entries, [1] = the assigned weight, [2] = the unassigned weight, [3] = the number of reads whose
 *   sample number is >= n_samples.  Those reads take no part in anything else: they are in no entry, no subject count and no
 *   weight total (subject[] and dist[], which count nothing, are written for them as for any read).
 * The answer is an exact integer function of the inputs: the same bytes from run to run and under smafa_set_prefilter /
 * smafa_set_zone_level / smafa_set_index and every SMAFA_ASSIGN_* setting.
 *
 * Checks, in this order, each SMAFA_ERR_INVALID with the argument named in smafa_last_error() and nothing written: a NULL handle;
 * a NULL query set (host form: NULL query_codes with n_queries > 0); NULL totals; max_div = SMAFA_NONE; n_samples = 0; NULL
 * entries with cap > 0; (launch form) a query set packed for another store; (host form) code bytes outside the alphabet, then a
 * sample number >= n_samples — checked on the host before any device work, the text names the first such read.  Behind the
 * checks totals[] is zeroed — the launch form's first enqueued operation, the host form's first store — and every other output
 * is written only by a call that succeeds.
 *
 * On the device (assign.hip.h): the reads go in spans of SMAFA_ASSIGN_SPAN (read when the handle is made; default 65 536, whole
 * 64s).  Each span is scanned as smafa_scan_launch(max_div, max_num_hits = 1) scans it — the rows are the subjects at each read's
 * minimum distance — into the handle's row list; where a span's rows do not fit, the list grows, doubling, up to
 * SMAFA_ASSIGN_ROWS_MAX rows (default: SMAFA_JOIN_SCRATCH_MAX's value), then the span is halved.  Only where 64 reads alone
 * overflow that limit — a store of millions of exact copies — the call fails: SMAFA_ERR_NOMEM, the count in smafa_last_error(),
 * and the handle stays usable.  One lane per row then takes the 64-bit minimum of (dist << 32 | subject) per read; one lane per
 * read looks the label up and writes a (label, sample) key and its weight; the device radix sort orders the m pairs over the
 * key bits in use; the first element of each run of equal keys is marked, an exclusive sum numbers the entries and a segmented
 * sum across each wave adds the weights, one 64-bit atomic per run and wave.  Reads of weight 0 get a key behind every other
 * and are cut off with the tail.  Fewer than 2^31 reads per call (the device sort's item limit).  Handle-owned scratch: 36 B per
 * read besides the row list.
 *
 * smafa_db_assign_launch: device-resident form.  d_labels = n_subjects uint32 or NULL; d_samples, d_weights = n_queries uint32 or
 * NULL; d_subject, d_dist = n_queries uint32 or NULL (not wanted); d_subject_counts = n_subjects uint64 or NULL; d_entries = cap
 * smafa_table_entry (NULL with cap = 0 counts only); d_totals = 4 uint64.  totals[0] is exact at any capacity and the first cap
 * entries IN TABLE ORDER are stored; the entries from totals[0] up to min(cap, n_queries) are zeroed, none behind that is touched.  Like smafa_db_self_launch the call synchronises the handle's stream between its spans and
 * once at its end.  smafa_last_scan_ms / smafa_last_call_stats hold the device time and launches of all its spans and of its own
 * passes; smafa_last_call_kernels lists the scan-family instantiations the call launched, then assign::init_kernel,
 * best_kernel (some row was listed), bin_kernel, heads_kernel and fold_kernel (no read at all: init_kernel alone).
 *
 * smafa_db_assign: host form; it makes and destroys a query set of its own.  More than cap entries: SMAFA_ERR_CAPACITY, totals[]
 * written (totals[0] = the entries needed), nothing else; nothing is kept for the retry.
 */
typedef struct {
    uint32_t label;
    uint32_t sample;
    uint64_t count;
} smafa_table_entry;
int smafa_db_assign_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, const void *d_labels /* n_subjects uint32, may be NULL */, const void *d_samples /* n_queries uint32, may be NULL */, uint32_t n_samples, const void *d_weights /* n_queries uint32, may be NULL */, void *d_subject /* n_queries uint32, may be NULL */, void *d_dist /* n_queries uint32, may be NULL */, void *d_subject_counts /* n_subjects uint64, may be NULL */, void *d_entries /* cap smafa_table_entry; NULL with cap == 0 counts only */, uint64_t cap, void *d_totals /* 4 uint64 */);
int smafa_db_assign(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, const uint32_t *labels, const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, uint32_t *subject, uint32_t *dist, uint64_t *subject_counts, smafa_table_entry *entries, uint64_t cap, uint64_t totals[4]);

/* ------------------------------------------------- classification: reads given the LCA of their best hits and counted */
/*
 * What SingleM does with the rows of `smafa query`: each read takes the lowest common ancestor (LCA) of the lineages of its
 * equally-best hits.  The abundance table above assigns a read to ONE subject; a read equally near two genera belongs to their
 * common family, not to whichever was appended first.  Not in the reference.
 * Inputs: the store's n subjects; m reads (a resident query set, or code rows); a bound max_div (required); slack >= 0; lineage,
 * n x n_ranks uint32, row-major, 1 <= n_ranks <= 16: lineage[i][r] is the id of subject i's taxon at rank r, rank 0 the most
 * general, SMAFA_NONE = "not classified at this rank or below" (a row is read up to its first SMAFA_NONE; a row that begins with
 * one has no lineage); samples, n_samples and weights as smafa_db_assign takes them.
 * Per read q:
 *   d(q)      the smallest distance of any subject within max_div.
 *   B(q)      the subjects s with dist(q, s) <= min(d(q) + slack, max_div): slack 0 — the equally-best hits.
 *   anchor(q) the smallest subject number among those at d(q): subject[q], with dist[q] = d(q) — smafa_db_assign's subject and
 *             dist, byte for byte.
 *   cp(a, s)  the number of leading ranks r with lineage[a][r] == lineage[s][r] != SMAFA_NONE.
 *   depth[q]  the minimum over s in B(q) of cp(anchor, s).  s = anchor is included, so an anchor classified to 3 ranks caps the
 *             depth at 3.  Where the ids form a tree this is the depth of the LCA of B(q): every member's lineage passes through
 *             the anchor's up to the rank at which it leaves it, so ONE minimum per read decides — no per-rank state.
 *   taxon[q]  lineage[anchor][depth - 1] where depth > 0; SMAFA_TAXON_ROOT (0xfffffffe) where depth is 0; SMAFA_NONE where no
 *             subject is within max_div (or the store is empty) — then subject, dist and depth are SMAFA_NONE too and ties is 0.
 *   ties[q]   |B(q)|.
 * The call compares ids rank by rank and asks nothing else of them.  Ids are compared WITHOUT their ancestors: two different
 * nodes that carry one id (a genus name under two families, say) are one taxon in the table.  Giving every node an id of its
 * own — interning (parent id, name), as `smafa classify` does — is the caller's affair.
 *   The TABLE: one smafa_table_entry {label = taxon, sample, count = the uint64 sum of weights} per (taxon, sample) that holds a
 *   read of weight > 0, ordered by (taxon, sample) ascending: SMAFA_TAXON_ROOT sorts behind every taxon, SMAFA_NONE (the
 *   unassigned reads) last.  Weight 0, a sample number >= n_samples and a short cap are handled exactly as by smafa_db_assign.
 *   totals[0] = the number of entries, [1] = the assigned weight (the root's included), [2] = the unassigned weight, [3] = the
 *   number of reads whose sample number is >= n_samples (they take no part in anything else; their per-read outputs are
 *   written), [4] = the weight placed on the root, [5] = the number of reads with ties > 1 (of any weight, [3]'s excepted).
 * The answer is an exact integer function of the inputs: the same bytes from run to run and under smafa_set_prefilter /
 * smafa_set_zone_level / smafa_set_index and every SMAFA_ASSIGN_* setting.
 *
 * Checks, in this order, each SMAFA_ERR_INVALID with the argument named in smafa_last_error() and nothing written: a NULL handle;
 * a NULL query set (host form: NULL query_codes with n_queries > 0); NULL totals; max_div = SMAFA_NONE; n_samples = 0; NULL
 * entries with cap > 0; n_ranks outside 1 .. 16; NULL lineage for a store that has subjects; (launch form) a query set packed
 * for another store; (host form) code bytes outside the alphabet, then a sample number >= n_samples, then the lineage — the
 * value SMAFA_TAXON_ROOT anywhere, or an id behind a SMAFA_NONE in its row — each on the host before any device work, the text
 * names the first such place.  The launch form does not look at the lineage: it reads each row up to its first SMAFA_NONE.
 * Behind the checks totals[] is zeroed — the launch form's first enqueued operation, the host form's first store — and every
 * other output is written only by a call that succeeds.
 *
 * On the device (classify.hip.h): smafa_db_assign's spans, row list and span rule (SMAFA_ASSIGN_SPAN, SMAFA_ASSIGN_ROWS_MAX).
 * With slack 0 a span is scanned as smafa_scan_launch(max_div, max_num_hits = 1) scans it; with slack > 0 as
 * smafa_scan_launch(max_div, SMAFA_NONE): every row within the bound.  A span whose rows do not fit is scanned again with the
 * list doubled, then halved, before any kernel of the call has seen it; 64 reads that alone overflow the limit fail the call:
 * SMAFA_ERR_NOMEM, and the handle stays usable.  Per taken span the table's 64-bit minimum (assign::best_kernel), then one lane
 * per row compares the row's lineage with the anchor's and the rows of one read that sit side by side in a wave are reduced
 * first: one 32-bit atomic minimum (depth) and one atomic add (ties) per run and wave.  Then one lane per read writes the
 * outputs and the (taxon, sample) key, and the table's sort, heads, exclusive sum and segmented sum follow unchanged.  Fewer
 * than 2^31 reads per call.  Handle-owned scratch: 48 B per read besides the row list.
 *
 * smafa_db_classify_launch: device-resident form.  d_lineage = n_subjects x n_ranks uint32 (NULL for an empty store); d_samples,
 * d_weights = n_queries uint32 or NULL; d_subject, d_dist, d_taxon, d_depth, d_ties = n_queries uint32 or NULL (not wanted);
 * d_entries = cap smafa_table_entry (NULL with cap = 0 counts only); d_totals = 6 uint64.  totals[0] is exact at any capacity and
 * the first cap entries IN TABLE ORDER are stored; the entries from totals[0] up to min(cap, n_queries) are zeroed, none behind
 * that is touched.  The call synchronises the handle's stream between its spans and at its end.  smafa_last_scan_ms /
 * smafa_last_call_stats hold the device time and launches of all its spans and of its own passes; smafa_last_call_kernels lists
 * the scan-family instantiations the call launched, then classify::start_kernel, assign::best_kernel and classify::agree_kernel
 * (some row was listed), classify::key_kernel, assign::heads_kernel and assign::fold_kernel (no read at all: start_kernel alone).
 *
 * smafa_db_classify: host form; it makes and destroys a query set of its own.  More than cap entries: SMAFA_ERR_CAPACITY,
 * totals[] written (totals[0] = the entries needed), nothing else; nothing is kept for the retry.
 */
int smafa_db_classify_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, uint32_t slack, const void *d_lineage /* n_subjects x n_ranks uint32 */, uint32_t n_ranks, const void *d_samples /* n_queries uint32, may be NULL */, uint32_t n_samples, const void *d_weights /* n_queries uint32, may be NULL */, void *d_subject /* n_queries uint32, may be NULL */, void *d_dist /* may be NULL */, void *d_taxon /* may be NULL */, void *d_depth /* may be NULL */, void *d_ties /* may be NULL */, void *d_entries /* cap smafa_table_entry; NULL with cap == 0 counts only */, uint64_t cap, void *d_totals /* 6 uint64 */);
int smafa_db_classify(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, uint32_t slack, const uint32_t *lineage, uint32_t n_ranks, const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, uint32_t *subject, uint32_t *dist, uint32_t *taxon, uint32_t *depth, uint32_t *ties, smafa_table_entry *entries, uint64_t cap, uint64_t totals[6]);

/* ------------------------------------------------- rows out of a store: a subset of it as a new store, its sequences back */
/* Every other call answers "which of the store's sequences do I want?"; these two act on the answer, on the device.
 *
 * smafa_db_subset_launch: keep[] holds one uint32 per subject, non-zero: keep; invert != 0 turns it into a drop list (the flags
 * of smafa_db_self_chimeras can be passed as they are).  *out is a NEW handle on the same device, with the same alphabet and
 * seq_len, the source's layout (its column order and per-column code tables copied, not chosen again) and the source's plane
 * count (a nucleotide store that held an N stays 3-plane even if no N survives); its knobs are read from the environment as
 * smafa_db_create reads them, and it has a stream of its own.  The kept subjects are renumbered 0 .. k-1 in ascending old number;
 * old_of_new[new] = old where the array is given.  The result has no index.  For every call of this header it is
 * indistinguishable from a store made by smafa_db_create and ONE smafa_db_append of the kept rows' codes in ascending old number:
 * the same subject numbers, distances and row order (the one exception is the choice among equal-weight forest edges, which is
 * free anyway).  The rows keep the source's position order — deleting rows from a sorted run leaves it sorted, so nothing is
 * sorted again — every run of the source keeps its kept rows and its "sorted", runs left without rows disappear, and the
 * quarter rule of the re-sort counts the kept rows outside the source's first run where that run is sorted, else all k.  The
 * zone words of the result are computed from its own tiles.  k == 0 gives a valid empty store with the layout set; a source
 * without rows accepts keep == NULL.
 * The SOURCE is not modified: its generation, block index, join state, retry rows and captured graph stay as they were.
 * The work runs on db's current stream and is complete when the call returns (k is needed on the host: smafa_db_consensus_launch
 * is the precedent); its kernels are in smafa_last_call_kernels(db), its device time in smafa_last_call_stats(db).
 * Checks, in this order: db, out (then *out = NULL), n_kept (then *n_kept = 0), keep unless the store is empty, and a store of
 * 2^31 rows or more is SMAFA_ERR_INVALID (the device scan counts in an int).  On any failure *out stays NULL and nothing is
 * leaked; a failed allocation is SMAFA_ERR_NOMEM and leaves no stale HIP error behind for the source's next launch.
 * smafa_db_subset: the same from host arrays; keep: n_subjects entries; old_of_new (or NULL): cap entries — cap < k with
 * old_of_new != NULL is SMAFA_ERR_CAPACITY with *n_kept = k and *out == NULL (cap is not read where old_of_new is NULL).
 *
 * smafa_db_rows_launch: the code bytes of m subjects, m x seq_len bytes in source column order with source codes — what
 * smafa_db_append was given.  d_subjects: m subject numbers on the device, in any order, repeats allowed; NULL: the range
 * first .. first + m - 1 (first is not read where a list is given).  A listed number >= n_subjects gives a row of 0xff bytes and
 * reads nothing of the store.  Checks, in this order: db; m == 0 is SMAFA_OK and touches nothing; d_codes; a range that passes
 * the end of the store is SMAFA_ERR_INVALID.  Runs on db's current stream and is complete when the call returns; reported as
 * above.  The call may bring the self-join's position table up to date, as a join would; nothing else of the handle changes.
 * smafa_db_rows: the same to a host array; every listed number is checked on the host first and one >= n_subjects is
 * SMAFA_ERR_INVALID with a text that names the entry. */
int smafa_db_subset_launch(smafa_db *db, const void *d_keep /* n_subjects uint32 */, int invert, smafa_db **out, void *d_old_of_new /* n_subjects uint32, may be NULL */, uint64_t *n_kept /* host */);
int smafa_db_subset(smafa_db *db, const uint32_t *keep, int invert, smafa_db **out, uint32_t *old_of_new /* may be NULL */, uint64_t cap, uint64_t *n_kept);
int smafa_db_rows_launch(smafa_db *db, const void *d_subjects /* m uint32; NULL: first .. first+m-1 */, uint64_t first, uint64_t m, void *d_codes /* m * seq_len bytes */);
int smafa_db_rows(smafa_db *db, const uint32_t *subjects, uint64_t first, uint64_t m, uint8_t *codes);

/* ------------------------------------------------- abundance-peak clusters with given weights (the sizes of dereplicated sequences) */
/* smafa_db_self_peaks with one line changed: weight[i] = weights_in[i] + the sum of weights_in[j] over the OTHER subjects within
 * distance r of i.  Keys, parents, labels, n_peaks, the kept pair list, the two phases, the edges and the failures are those of
 * smafa_db_self_peaks; with every weight 1 the two calls give the same bytes.  A weight of 0 is allowed and is simply the lightest.
 * A sum of weights_in above 4294967295 is SMAFA_ERR_INVALID (no weight can wrap), found on the device before anything is weighed.
 * max_div >= seq_len with r >= seq_len: every weight is that sum.  A NULL weights_in is SMAFA_ERR_INVALID unless the store is
 * empty (checked behind the radius, in front of cap).
 * What the weights are for: smafa_db_self_peaks at radius 0 counts abundance through the pairs at distance 0, c(c-1)/2 kept pairs
 * for a sequence of c copies, and raw reads hold sequences of 10^5 copies.  Dereplicate them first (vsearch --derep_fulllength,
 * DADA2's derepFastq, numpy.unique: this library has no such call yet), store every distinct sequence once and pass the sizes.
 * With S the store of the distinct rows of R in the order of their first copies, old_of_new[u] = the first row of R that holds
 * sequence u, unique_of[i] = the sequence of row i and sizes[u] = its copies, the peaks of S under weights_in = sizes are the peaks
 * of R, exactly: labels_R[i] == old_of_new[labels_S[unique_of[i]]] and weights_R[i] == weights_S[unique_of[i]] for every i, and
 * n_peaks is the same — a raw row's heaviest neighbour is always the first of a sequence's copies, and the new numbers keep the
 * order of those, so ties break the same way.  The join of S keeps no pair at distance 0.
 * The kernels are the plain call's: the weights are an argument of smafa_pk::init_peaks_kernel (which copies and sums them where
 * it writes ones) and of smafa_pk::weigh_keep_kernel, and smafa_last_call_kernels reads as for smafa_db_self_peaks.  What the
 * call adds: one host wait behind the first launch (the sum is checked before anything is weighed) and, where r >= seq_len, one
 * more launch of init_peaks_kernel, which then writes the sum into every weight; otherwise the launch count is the plain call's. */
int smafa_db_self_peaks_weighted_launch(smafa_db *db, uint32_t max_div, uint32_t radius, const void *d_weights_in /* n_subjects uint32 */, void *d_labels, void *d_parents /* may be NULL */, void *d_weights /* may be NULL */, void *d_n_peaks /* uint64 */);
int smafa_db_self_peaks_weighted(smafa_db *db, uint32_t max_div, uint32_t radius, const uint32_t *weights_in, uint32_t *labels, uint32_t *parents, uint32_t *weights, uint64_t cap, uint64_t *n_peaks);
/* smafa_peaks_weighted: smafa_peaks with the weights of a file, "i<TAB>weight" lines as for smafa_chimeras (further columns are
 * ignored, a sequence without a line weighs 0, "-": stdin).  SMAFA_ERR_INVALID: a NULL path or weights_path. */
int smafa_peaks_weighted(const char *db_path, uint32_t max_divergence, uint32_t radius, const char *weights_path, int out_fd, int device);

/* ------------------------------------------------- the same store on several GPUs */
/*
 * "queries sharded across the handle's devices internally".  A group is ONE subject store replicated on every
 * entry of `devices` (an entry may repeat: several handles on one GPU); what is sharded is the reference's per-query loop,
 * src/lib.rs:232-318, around get_distances (:238) — it carries no state between queries but the running query number.
 * smafa_group_scan_hits has the contract of smafa_scan_hits (same bounds, same order, same grow-and-retry): the batch
 * is cut into ndev contiguous blocks, block g is scanned on devices[g] by its own host thread, and the blocks' rows are
 * concatenated in block order, so the rows do not depend on ndev.  No collective: replicas never exchange anything.
 * One group = one owner thread at a time.  smafa_query_multi is a caller of this.
 */
int smafa_group_create(smafa_group **out, const int *devices, int ndev, int alphabet, uint32_t seq_len);
/* every member from the same packed store file (smafa_db_load per device; the file is mapped once) */
int smafa_group_load(smafa_group **out, const int *devices, int ndev, const char *path);
/* push_encoding x n on every replica (src/lib.rs:91-111); subject indices agree across the members */
int smafa_group_append(smafa_group *grp, const uint8_t *codes, uint64_t n);
int smafa_group_scan_hits(smafa_group *grp, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div,
                          uint32_t max_num_hits, smafa_hit *out, uint64_t cap, uint64_t *n_out);
/* smafa_db_build_index on every member, side by side (each replica keeps its own index on its device) */
int smafa_group_build_index(smafa_group *grp, uint32_t max_divergence);
int smafa_group_size(const smafa_group *grp);
/* member `index` (borrowed; owned by the group): for smafa_db_info, the tuning knobs, or device-resident launches.
 * Rows are appended through smafa_group_append only (the replicas must stay identical); never destroy a member. */
smafa_db *smafa_group_member(smafa_group *grp, int index);
void smafa_group_destroy(smafa_group *grp); /* NULL-safe */

/* -------------------------------------------------------- host-side selection */
/*
 * The row-selection rules of query (src/lib.rs:241-315) applied to a hit list already ordered by
 * (query, dist, subject) that holds, per query, at least every subject within min(max_div, kth).
 * subject_codes (n_subjects rows of seq_len) is needed only for limit_per_sequence (adjacent equal
 * strings, src/lib.rs:269-289).  n_queries = number of queries the hit list covers (query ids
 * 0..n_queries-1); a query with no hit at all while max_div is SMAFA_NONE means an empty store.
 * Returns SMAFA_ERR_PANIC for the inputs the reference panics on (empty store, k = 0,
 * limit_per_sequence without max_num_hits > 1).  Output rows are in print order.
 */
int smafa_select_rows(const smafa_hit *hits, uint64_t n_hits, uint64_t n_queries, uint64_t n_subjects,
                      const uint8_t *subject_codes, uint32_t seq_len, uint32_t max_div, uint32_t max_num_hits,
                      uint32_t limit_per_sequence, smafa_hit *rows, uint64_t cap, uint64_t *n_rows);

/* Print rows the way query does (src/lib.rs:292,310): "{query_offset + query}\t{subject}\t{dist}\t{subject string}\n"
 * per row, to out_fd.  For hosts that select rows themselves (the multi-GPU driver on rank 0). */
int smafa_write_rows(const smafa_hit *rows, uint64_t n_rows, const uint8_t *subject_codes, uint64_t n_subjects,
                     uint32_t seq_len, int alphabet, uint32_t query_offset, int out_fd);

/* ------------------------------------------------------------------ DB file */
/* Serialise / parse the reference's v2 DB file (postcard wire format of WindowSet,
 * src/lib.rs:54-60,161-162,208-218).  NT only.  smafa_dbfile_write: codes -> file bytes identical to
 * the reference's makedb.  smafa_dbfile_read: file -> malloc'd code rows (free with smafa_free);
 * a version other than 2 fails with the reference's "Unsupported db file version" text.
 * Version 3 is this build's extension container for amino-acid stores (alphabet byte + raw code rows). */
int smafa_dbfile_write(const char *path, int alphabet, const uint8_t *codes, uint64_t n, uint32_t seq_len);
int smafa_dbfile_read(const char *path, int *alphabet, uint8_t **codes, uint64_t *n, uint32_t *seq_len);
/* Read a FASTA/FASTQ(+gzip) file of equal-length records into malloc'd code rows (free with smafa_free) —
 * parse_fastx_file + from_bytes per record (src/lib.rs:221,235).  Fails like the reference on a byte outside
 * the alphabet (message of src/lib.rs:38-41); records of unequal length fail with SMAFA_ERR_PANIC. */
int smafa_fastx_load(const char *path, int alphabet, uint8_t **codes, uint64_t *n, uint32_t *seq_len);
/* The same, stopping quietly at the first offending record: returns the rows before it, and in *pending the code
 * smafa_fastx_load would have failed with (message in smafa_last_error()) or SMAFA_OK.  For hosts that — like the
 * reference's loop, src/lib.rs:232-318 — answer the queries in front of a bad record before they fail. */
int smafa_fastx_load_partial(const char *path, int alphabet, uint8_t **codes, uint64_t *n, uint32_t *seq_len, int *pending);
/* One PART of a plain FASTA/FASTQ file, for hosts that shard a query file over processes: the records that start in this
 * part's byte range (part p of `parts`: the first record start at or after byte size*p/parts up to the next part's) — the
 * parts partition the records in file order and a process reads only its own bytes.  *usable = 0 (and no rows): the file
 * cannot be taken in parts (gzip, a cut that did not hold, a malformed record) — load the whole file instead.  *seq_len =
 * the length of the part's first record; *pending as in smafa_fastx_load_partial.  (parse_fastx_file + the loop of
 * src/lib.rs:221,232-235, one share of it.) */
int smafa_fastx_load_part(const char *path, int alphabet, uint32_t part, uint32_t parts, uint8_t **codes, uint64_t *n,
                          uint32_t *seq_len, int *pending, int *usable);
void smafa_free(void *p);

/* ------------------------------------------- drivers: the crate's pub fns */
/* makedb(subject_fasta, db_path) — src/lib.rs:137-165.  Host only (no GPU needed). */
int smafa_makedb(const char *subject_fasta, const char *db_path, int alphabet);
/* makedb with the packed store file as output: the subjects are packed on `device` (the layout is the one a query
 * would build) and saved with smafa_db_save.  device < 0, or no GPU visible: packed by host threads instead — the same
 * bytes (host/layout.cpp restates the device's packing; the two files are compared in tests/test_gpu_layout.py). */
int smafa_makedb_packed(const char *subject_fasta, const char *db_path, int alphabet, int device);
/* query(db_path, query_fasta, max_divergence, max_num_hits, limit_per_sequence) — src/lib.rs:198-325.
 * Options use SMAFA_NONE for None.  TSV rows go to out_fd (the reference prints to stdout). */
int smafa_query(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t max_num_hits,
                uint32_t limit_per_sequence, int out_fd, int device);
/* The same query spread over several GPUs of one node by ONE process ("queries sharded across the handle's
 * devices internally"): one handle per entry of `devices` (an entry may repeat: several handles on one GPU), the store
 * replicated on each, every chunk of queries cut into ndev contiguous blocks scanned by one host thread per handle,
 * rows printed in block order.  The loop being sharded is src/lib.rs:232-318, which carries no state between queries
 * but the running query number, so the bytes written do not depend on ndev.  No collective, no torch. */
int smafa_query_multi(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t max_num_hits,
                      uint32_t limit_per_sequence, int out_fd, const int *devices, int ndev);
/* ---- `query` for hosts that run ONE PROCESS PER GPU (smafa_amd/dist.py over torch.distributed / RCCL, or MPI) ----
 * The loop of src/lib.rs:232-318 carries no state between records but the running query number, so the query FILE is cut
 * into `parts` contiguous shares in rank order.  A process opens the DB once (a packed store file is mapped and copied to
 * HBM: no decode, no host code rows), answers its share — reading ONLY its byte range of a plain FASTA/FASTQ file — and
 * rank 0 prints the gathered rows, decoding subject strings for the hit rows only.
 *   smafa_qsession_scan_part: rows (malloc'd, free with smafa_free) are numbered from 0 within the share and already
 *   selected (src/lib.rs:241-315); *n_queries = records of the share that were answered; *pending = SMAFA_OK or the code of
 *   the first record the reference's loop fails on inside this share (text in smafa_last_error()): the caller prints the
 *   rows of the ranks up to and including the first such rank, then fails with that text.
 *   whole_file = 0: the share is the records that start in this part's byte range; *n_before = UINT64_MAX (the caller
 *   adds up the counts of the ranks in front); *retry_whole = 1 (and nothing else) when the file cannot be taken in parts
 *   (gzip, a cut that did not hold, a malformed record): EVERY rank must then call again with whole_file = 1 — the whole
 *   file is parsed, the share is block [part*Q/parts, (part+1)*Q/parts) of its Q usable records and *n_before its start. */
typedef struct smafa_qsession smafa_qsession;
int smafa_qsession_open(smafa_qsession **out, const char *db_path, int device); /* device < 0: no store in HBM (printing only) */
int smafa_qsession_info(const smafa_qsession *s, uint64_t *n_subjects, uint32_t *seq_len, int *alphabet);
int smafa_qsession_scan_part(smafa_qsession *s, const char *query_fasta, uint32_t max_divergence, uint32_t max_num_hits,
                             uint32_t limit_per_sequence, uint32_t part, uint32_t parts, int whole_file, smafa_hit **rows,
                             uint64_t *n_rows, uint64_t *n_queries, uint64_t *n_before, int *pending, int *retry_whole);
int smafa_qsession_write(smafa_qsession *s, const smafa_hit *rows, uint64_t n_rows, int out_fd);
void smafa_qsession_close(smafa_qsession *s); /* NULL-safe */
/* cluster(input_fasta, max_divergence, print_stream) — src/cluster.rs:13-94. */
int smafa_cluster(const char *input_fasta, uint32_t max_divergence, int out_fd, int device, int alphabet);
/* The same clustering spread over `world` processes, one GPU each (cluster mode): every rank reads
 * the whole input and keeps a replica of the centroid store on its own device; each batch of unseen records is
 * split into contiguous slices, rank r scans slice r, and the per-record results are exchanged through
 * `allgather` twice per batch (nearest old centroid: 8 bytes per record; in-range (record, candidate) rows:
 * 12 bytes each).  Every rank then resolves the batch identically and appends the same new centroids to its
 * replica — there is no broadcast.  Rank 0 writes the reference's output bytes to out_fd; other ranks write
 * nothing.  The result does not depend on `world`.
 * `allgather(ctx, send, send_bytes, &recv, &recv_bytes)` must return 0 and leave in *recv the blocks of ALL
 * ranks concatenated in rank order (block sizes differ between ranks); the buffer stays valid until the next
 * call.  The library never touches the transport: the caller supplies RCCL (torch.distributed in
 * smafa_amd/dist.py), MPI, ... */
typedef int (*smafa_allgather_fn)(void *ctx, const void *send, uint64_t send_bytes, const void **recv,
                                  uint64_t *recv_bytes);
int smafa_cluster_sharded(const char *input_fasta, uint32_t max_divergence, int out_fd, int device, int alphabet,
                          uint32_t rank, uint32_t world, smafa_allgather_fn allgather, void *ctx);
/* The same clustering over several GPUs of one node by ONE process (no torch, no collective library): one host thread per entry
 * of `devices` (entries may repeat) plays a rank of smafa_cluster_sharded — its own replica of the centroid store, its slice of
 * every batch — the input is parsed and de-duplicated once for all of them, and the two exchanges per batch go through memory.
 * Output bytes do not depend on ndev (src/cluster.rs:13-94 semantics). */
int smafa_cluster_multi(const char *input_fasta, uint32_t max_divergence, int out_fd, const int *devices, int ndev, int alphabet);
/* `smafa pairs` (not in the reference): the DB file (version 2 / 3 or a packed store file, as smafa_query takes them) is
 * loaded on `device`, and every pair of its subjects within max_divergence (smafa_db_self_hits) is written to out_fd as
 * "{i}\t{j}\t{distance}\n", i < j, in (i, distance, j) order. */
int smafa_pairs(const char *db_path, uint32_t max_divergence, int out_fd, int device);
/* `smafa pairs --since ROW` (not in the reference): the same DB, and the pairs whose larger subject number is >= first_row
 * (smafa_db_self_hits_since) in the same format and order: exactly the lines of smafa_pairs with j >= first_row.  first_row
 * above the number of subjects is SMAFA_ERR_INVALID. */
int smafa_pairs_since(const char *db_path, uint64_t first_row, uint32_t max_divergence, int out_fd, int device);
/* `smafa components` (not in the reference): the DB file (version 2 / 3 or a packed store file), loaded on `device` as for
 * smafa_pairs, and per subject its label (smafa_db_self_components: the smallest subject number of its single-linkage
 * component at max_divergence) as "{i}\t{label}\n", in subject order, to out_fd.  An empty DB writes nothing. */
int smafa_components(const char *db_path, uint32_t max_divergence, int out_fd, int device);
/* `smafa components --levels` (not in the reference): the same DB, and per subject its label at every bound 0 ..
 * max_divergence (smafa_db_self_levels), "{i}\t{label_0}\t...\t{label_N}\n" in subject order.  Column t + 1 is the label
 * column of smafa_components at bound t.  An empty DB prints nothing. */
int smafa_component_levels(const char *db_path, uint32_t max_divergence, int out_fd, int device);
/* `smafa forest` (not in the reference): the same DB, and the minimum spanning forest of its subjects up to max_divergence
 * (smafa_db_self_forest), "{a}\t{b}\t{distance}\n" per edge, a < b, ordered by distance, then a, then b.  The lines with
 * distance <= t are the merge tree of `smafa components --max-divergence t`; which of several pairs of equal distance joins
 * two components may differ from run to run.  An empty DB prints nothing. */
int smafa_forest(const char *db_path, uint32_t max_divergence, int out_fd, int device);
/* `smafa forest --min-pts M` (not in the reference): the same DB, and the mutual-reachability forest of its subjects up to
 * max_divergence at min_pts (smafa_db_self_reach_forest), "{a}\t{b}\t{weight}\n" per edge, a < b, ordered by weight, then a,
 * then b; with cores != 0 (`--cores`) the core distance of every subject instead, "{i}\t{core}\n" in subject order, -1 for a
 * row that is sparse at the bound: the k-distance plot.  An empty DB prints nothing. */
int smafa_reach_forest(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int cores, int out_fd, int device);
/* `smafa stable` (not in the reference): the same DB, and per subject the label of its stable cluster (smafa_db_self_stable at
 * max_divergence, min_pts and min_cluster_size), "{i}\t{label}\n" in subject order, -1 for noise; with joined != 0
 * (`--joined`) a third column, the level at which the subject joined its cluster, -1 for noise.  An empty DB prints nothing. */
int smafa_stable(const char *db_path, uint32_t max_divergence, uint32_t min_pts, uint32_t min_cluster_size, int joined, int out_fd, int device);
/* `smafa consensus` (not in the reference): the same DB and a labels file — "{i}\t{label}[\t...]\n" per subject exactly as
 * `components`, `density`, `peaks` and `stable` print them, further columns ignored, -1 for SMAFA_NONE; labels_path "-" is
 * stdin.  Line j must carry i = j and there must be n_subjects lines: anything else — a label that is neither
 * -1 nor below n_subjects included — is SMAFA_ERR_INVALID with a text that names the line (exit status 1).  Per cluster, in ascending label order (smafa_db_consensus),
 * "{label}\t{size}\t{nearest}\t{max_div}\t{SEQUENCE}\n": max_div the greatest div among the cluster's members, SEQUENCE
 * smafa_decode of the consensus.  An empty DB prints nothing. */
int smafa_consensus(const char *db_path, const char *labels_path, int out_fd, int device);
/* `smafa density` (not in the reference): the same DB, and per subject its density-cluster label and its degree
 * (smafa_db_self_density at max_divergence and min_pts), "{i}\t{label}\t{degree}\n" in subject order; the label of a noise row
 * is printed as -1.  An empty DB prints nothing. */
int smafa_density(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int out_fd, int device);
/* `smafa peaks` (not in the reference): the same DB, and per subject its abundance-peak label, its parent and its weight
 * (smafa_db_self_peaks at max_divergence and radius), "{i}\t{label}\t{parent}\t{weight}\n" in subject order.  An empty DB
 * prints nothing. */
int smafa_peaks(const char *db_path, uint32_t max_divergence, uint32_t radius, int out_fd, int device);
/* `smafa chimeras` (not in the reference): the same DB, and per subject the verdict of the chimera check (smafa_db_self_chimeras
 * at max_divergence, radius and min_fold), "{i}\t{flag}\t{left_parent}\t{left_len}\t{right_parent}\t{right_len}\t{weight}\n" in
 * subject order, -1 for SMAFA_NONE.  weights_path NULL: the weights are counted at the radius.  Else a file of "{i}\t{weight}[\t...]\n"
 * lines ("-": stdin; further columns ignored; in any order; a subject without a line has weight 0); a line that is not of that
 * form, a second line for one subject or a subject number the DB does not have is SMAFA_ERR_INVALID with a text that names the
 * line (exit status 1).  An empty DB prints nothing. */
int smafa_chimeras(const char *db_path, uint32_t max_divergence, uint32_t radius, uint32_t min_fold, const char *weights_path, int out_fd, int device);
/* `smafa table` (not in the reference): the same DB, the reads of a FASTA/FASTQ(+gzip) file — of the store's length, or the call
 * fails as smafa_query does — and smafa_db_assign at max_divergence.  labels_path (or NULL: a subject's label is its own number):
 * the file `smafa consensus` reads, except that the file may end early — a subject without a line has label -1.  samples_path and
 * weights_path (or NULL): "{read}\t{value}[\t...]\n" lines over read numbers, in any order; a read without a line is in sample 0 /
 * weighs 1; n_samples = the largest sample number + 1.  "-" is stdin for at most one of the three.  A line that is not of that
 * form, a second line for one read or a read number the file does not have is SMAFA_ERR_INVALID with a text that names the line.
 * Output: "{label}\t{sample}\t{count}\n" per entry in table order, -1 for SMAFA_NONE; per_read != 0: "{read}\t{subject}\t{dist}\n"
 * per read instead, -1 in both columns for an unassigned read; per_sequence != 0: "{i}\t{count}\n" per subject
 * (subject_counts: what `smafa chimeras --weights -` reads).  per_read and per_sequence together are SMAFA_ERR_INVALID.  An empty
 * DB prints nothing. */
int smafa_table(const char *db_path, const char *query_fasta, uint32_t max_divergence, const char *labels_path, const char *samples_path, const char *weights_path, int per_read, int per_sequence, int out_fd, int device);
/* `smafa classify` (not in the reference): the same DB and reads file as `smafa table`, and smafa_db_classify at max_divergence
 * and slack.  taxonomy_path (required): "{i}\t{name};{name};...[\t...]\n" lines over subject numbers, in any order, rank 0 first;
 * names are trimmed of blanks (SingleM's "Root; d__Bacteria; ..." reads as it stands), further columns are ignored, a trailing
 * ';' or an empty second column adds no name; a subject without a line (or without a name) has no lineage.  More than 16 names
 * on a line, an empty name between two others, a rank-0 name "root" or "unassigned", a second line for one subject or a subject
 * number the DB does not have is SMAFA_ERR_INVALID with a text that names the line.  Ids are interned by (parent id, name) in order
 * of first appearance in the file, so every node has an id of its own and the table's order is a function of the file alone.
 * samples_path, weights_path (or NULL): as for smafa_table.  "-" is stdin for at most one of the three.
 * Output: "{lineage}\t{sample}\t{count}\n" per entry in table order, the lineage the names joined by ';' down to the node, "root"
 * for SMAFA_TAXON_ROOT, "unassigned" for SMAFA_NONE; per_read != 0: "{read}\t{subject}\t{dist}\t{ties}\t{depth}\t{lineage}\n" per
 * read instead, -1 for subject, dist and depth of an unassigned read.  An empty DB prints nothing. */
int smafa_classify(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t slack, const char *taxonomy_path, const char *samples_path, const char *weights_path, int per_read, int out_fd, int device);
/* `smafa subset` (not in the reference): the same DB, a list of sequence numbers and smafa_db_subset — keep_path: the sequences
 * to keep, or drop_path: the ones to drop; exactly one of the two is given (both or neither is SMAFA_ERR_INVALID), "-" is stdin.
 * The file holds one sequence number per line in its first column; further tab-separated columns are ignored, so the lines
 * another verb printed can be piped in behind a filter; duplicates are allowed.  A line that is not of that form or a number
 * the DB does not have is SMAFA_ERR_INVALID with a text that names the line.  out_path is written by smafa_db_save as a packed
 * store that every verb reads; out_fd gets "{new}\t{old}\n" per kept sequence. */
int smafa_subset(const char *db_path, const char *keep_path, const char *drop_path, const char *out_path, int out_fd, int device);
/* `smafa neighbours` (not in the reference): the same DB, and per subject its neighbours within max_divergence, nearest first,
 * at most max_num_hits of them (SMAFA_NONE: all) — smafa_db_self_neighbours, a degrees-only call and then the sized one —
 * "{i}\t{j}\t{dist}\n" per entry, both directions of every pair, ordered by (i, dist, j).  An empty DB prints nothing. */
int smafa_neighbours(const char *db_path, uint32_t max_divergence, uint32_t max_num_hits, int out_fd, int device);
/* count(paths) — src/lib.rs:378-398 (JSON to out_fd).  Host only. */
int smafa_count(const char *const *paths, uint64_t n_paths, int out_fd);

#ifdef __cplusplus
}
#endif
#endif

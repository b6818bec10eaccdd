// reach.hip.h — kernels of the MUTUAL-REACHABILITY forest of a resident store (engine.hip: smafa_db_self_reach_forest_launch):
// the tree HDBSCAN starts from.  The graph is the one of density.hip.h at every bound at once — vertices the store's subjects,
// edges the pairs within max_div whose ends are both not sparse — and an edge weighs
//     w = max(distance(a, b), core[a], core[b]),
// core[i] = the smallest t with ball(i, t) >= min_pts, ball(i, t) = 1 + the number of OTHER rows within t of row i (the row counts
// itself, equal rows at other numbers count: density.hip.h's degree[i] + 1 at bound t), SMAFA_NONE where there is none up to the
// bound (the row is SPARSE).  The result is a minimum spanning forest of that graph, as forest.hip.h gives one of the plain graph:
// edges {a, b, w}, a < b, ordered by w; for every t the edges with w <= t are acyclic and connect exactly the pairs within t
// whose ends are both core at t — the core rows' clusters of the density call at bound t, for every t from one join.
// The tenth consumer of a finished piece's scratch list, in a namespace of its own:
//   tally_keep_kernel   smafa_sf::keep_row, keep_pairs_kernel's loop body — per row the exactly-once rule keeps, the row moves to the
//                       handle's kept pair list while that has room — and, stored or not, the row is tallied at both ends:
//                       hist[a * E + dist]++, hist[b * E + dist]++ (exact at any capacity of the list, as the density call's degrees)
//   core_dist_kernel    one lane per subject: the running sum from 1 over the row's E tallies, core[i] = the first t at which it
//                       reaches min_pts, else `fallback`; the rows that are not sparse are counted
//   span_reach_kernel   smafa_sf::span_row, span_edges_kernel's loop body, with the weight above: one launch per class t, per row with w == t
//                       unite_won(a, b); the lane whose own CAS made the hook writes {min, max, w}
// smafa_sf::init_forest_kernel, unite_won and star_roots_kernel are used as they are; the union-find is components.hip.h's.
//
// Why the winners are a minimum forest of the WEIGHTED graph: forest.hip.h's argument with the class defined by w.  A win
// merges two distinct sets and every merge is one win (acyclic, at most n - 1 wins).  The classes run one after another with a
// kernel boundary between only_dist = t and t + 1, and w >= dist, so when class t starts every row of weight < t has its ends
// joined and parent[] holds exactly the components of the graph cut below t; a row of class t wins only if no path of lighter
// rows joins its ends.  core[] is final before the first class (a kernel boundary behind core_dist_kernel) and read-only after.
//
// No flags, no spinning, no hand-off between workgroups, no inline assembly: the only synchronisation is the atomics on parent[],
// hist[] and the running totals, and the kernel boundary.  Every load of parent[] inside the union is smafa_cc::load_parent.
#pragma once

#include "forest.hip.h"

namespace smafa_mr {

// Every kept row of smafa_sf::keep_row, stored or not, raises hist[a * E + dist] and hist[b * E + dist] (the join ran at bound
// E - 1: dist < E; the compare keeps a wrong row from writing outside hist[]).
struct TallyPerRow {
    uint32_t *hist;
    uint32_t E;
    __device__ __forceinline__ void operator()(const smafa_hit &h) const {
        if (h.dist < E) {
            atomicAdd(hist + (size_t)h.query * E + h.dist, 1u);
            atomicAdd(hist + (size_t)h.subject * E + h.dist, 1u);
        }
    }
};

__global__ __launch_bounds__(256) void tally_keep_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, smafa_hit *kept, unsigned long long cap,
                                                         unsigned long long *ctl, uint32_t *hist, uint32_t E) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;  // (uniform trip count per workgroup)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride)
        smafa_sf::keep_row(list, total, base + threadIdx.x, p0, S, R, order, pos_of, kept, cap, ctl, TallyPerRow{hist, E});
}

// Behind the join every tally is final (the kernel boundary; plain loads).  ball(i, t) = 1 + hist[i * E + 0 .. t]; core[i] = the
// first t at which it reaches min_pts, `fallback` where it does not up to E - 1: seq_len where max_div >= seq_len and the store
// has min_pts rows (every other row is within seq_len), SMAFA_NONE elsewhere.  cores: the caller's copy, or nullptr.  The rows
// that are not sparse are counted on *n_dense, one atomicAdd per wave.
__global__ __launch_bounds__(256) void core_dist_kernel(const uint32_t *__restrict__ hist, uint32_t n, uint32_t E, uint32_t min_pts,
                                                        uint32_t fallback, uint32_t *__restrict__ core, uint32_t *__restrict__ cores,
                                                        unsigned long long *n_dense) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool dense = false;
    if (i < n) {
        uint32_t found = fallback, ball = 1u;
        const uint32_t *mine = hist + (size_t)i * E;
        for (uint32_t t = 0; t < E; t++) {
            ball += mine[t];
            if (ball >= min_pts) {
                found = t;
                break;
            }
        }
        core[i] = found;
        if (cores) cores[i] = found;
        dense = found != SMAFA_NONE;
    }
    const unsigned long long mask = __ballot(dense);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(n_dense, (unsigned long long)__builtin_popcountll(mask));
}

// The rows with max(dist, core[a], core[b]) == t for smafa_sf::span_row — a row with dist > t passes by before any gather,
// because w >= dist.  SMAFA_NONE (a sparse end) matches no class.
struct ReachClass {
    const uint32_t *__restrict__ core;
    uint32_t t;
    __device__ __forceinline__ bool maybe(uint32_t dist) const { return dist <= t; }
    __device__ __forceinline__ bool is(uint32_t dist, uint32_t a, uint32_t b) const { return max(dist, max(core[a], core[b])) == t; }
};

__global__ __launch_bounds__(256) void span_reach_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ core, uint32_t *parent, uint32_t only_dist,
                                                         smafa_hit *edges, unsigned long long cap, unsigned long long *n_edges) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;  // (uniform trip count per workgroup)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride)
        smafa_sf::span_row(list, total, base + threadIdx.x, p0, S, R, order, parent, edges, cap, n_edges, ReachClass{core, only_dist});
}

}  // namespace smafa_mr

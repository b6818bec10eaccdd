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
//   tally_keep_kernel   smafa_sf::keep_pairs_kernel's body — per row the exactly-once rule keeps, the row {a, b, dist} moves to the
//                       handle's kept pair list while that has room — and, stored or not, the row is tallied at both ends:
//                       hist[a * E + dist]++, hist[b * E + dist]++ (exact at any capacity of the list, as the density call's degrees)
//   core_dist_kernel    one lane per subject: the running sum from 1 over the row's E tallies, core[i] = the first t at which it
//                       reaches min_pts, else `fallback`; the rows that are not sparse are counted
//   span_reach_kernel   smafa_sf::span_edges_kernel with the weight above: one launch per weight class t, per row with w == t
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

// The piece's list as smafa_sf::keep_pairs_kernel receives it, and its rule: a row is kept iff position(query row) <
// pos_of[subject].  A kept row {a, b, dist} in subject numbers goes to kept[first + ...], one reservation per wave on ctl[0]
// (the kept total); rows past cap are counted and not stored.  Every kept row, stored or not, raises hist[a * E + dist] and
// hist[b * E + dist] (the join ran at bound E - 1: dist < E; the compare keeps a wrong row from writing outside hist[]).
__global__ __launch_bounds__(256) void tally_keep_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, smafa_hit *kept, unsigned long long cap,
                                                         unsigned long long *ctl, uint32_t *hist, uint32_t E) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        const unsigned long long i = base + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool keep = false;
        if (i < total) {
            h = list[i];
            const uint32_t qpos = p0 + (h.query % R) * S + h.query / R;
            keep = qpos < pos_of[h.subject];
            if (keep) {
                h.query = order[qpos];  // (another position than the subject's: another subject number)
                if (h.dist < E) {
                    atomicAdd(hist + (size_t)h.query * E + h.dist, 1u);
                    atomicAdd(hist + (size_t)h.subject * E + h.dist, 1u);
                }
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (mask == 0ull) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(ctl, (unsigned long long)__builtin_popcountll(mask));
        first = smafa::shfl_u64(first, 0);
        const unsigned long long slot = first + smafa::lanes_below(mask);
        if (keep && slot < cap) kept[slot] = h;
    }
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

// One weight class: the rows with max(dist, core[a], core[b]) == only_dist, all others pass by — a row with dist > only_dist
// before any gather, because w >= dist.  The two list forms of smafa_sf::span_edges_kernel: order != nullptr, a raw piece list;
// order == nullptr, the kept list in subject numbers.  SMAFA_NONE (a sparse end) matches no class.  Self-pairs are skipped, equal
// parents are one set already, and a lane that won writes {min, max, w} to edges[first + ...], one reservation per wave on
// *n_edges; cap = n - 1 is never reached (forest.hip.h), the compare keeps a wrong parent[] from writing past the caller's buffer.
__global__ __launch_bounds__(256) void span_reach_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ core, uint32_t *parent, uint32_t only_dist,
                                                         smafa_hit *edges, unsigned long long cap, unsigned long long *n_edges) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        const unsigned long long i = base + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool won = false;
        if (i < total) {
            h = list[i];
            if (h.dist <= only_dist) {
                const uint32_t a = order ? order[p0 + (h.query % R) * S + h.query / R] : h.query, b = h.subject;
                if (a != b && max(h.dist, max(core[a], core[b])) == only_dist &&
                    smafa_cc::load_parent(parent, a) != smafa_cc::load_parent(parent, b))
                    won = smafa_sf::unite_won(parent, a, b);
                h.query = min(a, b);
                h.subject = max(a, b);
                h.dist = only_dist;
            }
        }
        const unsigned long long mask = __ballot(won);
        if (mask == 0ull) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(n_edges, (unsigned long long)__builtin_popcountll(mask));
        first = smafa::shfl_u64(first, 0);
        const unsigned long long slot = first + smafa::lanes_below(mask);
        if (won && slot < cap) edges[slot] = h;
    }
}

}  // namespace smafa_mr

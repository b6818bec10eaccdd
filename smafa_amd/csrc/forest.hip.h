// forest.hip.h — kernels of the minimum spanning FOREST of a resident store (engine.hip: smafa_db_self_forest_launch): the
// merge tree of single linkage.  The graph is the one of components.hip.h and levels.hip.h — vertices the store's subjects,
// edges the pairs within a bound, an edge's weight its distance — and the result is a list of edges {a, b, dist}, a < b,
// ordered by dist, that is a minimum spanning forest of it: for every t the edges with dist <= t are acyclic and their
// connected components are exactly the components at bound t; level_ends[t] = their number = n - n_components[t].  The
// seventh consumer of a finished piece's scratch list, next to join_filter_kernel (join.hip.h), link_rows_kernel
// (components.hip.h), hook_levels_kernel (levels.hip.h), count_keep_kernel (density.hip.h), weigh_keep_kernel (peaks.hip.h)
// and mirror_pack_kernel (neighbours.hip.h), in a namespace of its own:
//   init_forest_kernel   parent[i] = i
//   keep_pairs_kernel    per row of a piece's list that the exactly-once rule keeps: the row {a, b, dist} moves to the handle's
//                        KEPT PAIR LIST while that has room (nothing is united during the join)
//   span_edges_kernel    one launch per weight class t: per row with dist == t, unite_won(a, b); the lane whose own CAS made
//                        the hook writes the row to edges[]
//   star_roots_kernel    bounds no two rows can exceed (max_div >= seq_len): every surviving root r != 0 gets the edge
//                        (0, r, seq_len), and level_ends[seq_len ..] = n - 1
// Distances are integers 0 .. D, so Kruskal's algorithm runs by weight class: the classes one after another, the edges of a
// class in any order — here concurrently.
//
// The union-find is the one of components.hip.h (smafa_cc::find_root and load_parent as they are: the larger root goes under
// the smaller by atomicCAS on the larger root's own slot, path halving by atomicMin, every load of parent[] an agent-scope
// relaxed atomic load; slots only go down, a stale value is still an ancestor in the same set, the CAS alone decides whether a
// node is still a root).  New here is unite_won: smafa_cc::unite's loop, returning whether THIS call's CAS made the hook.
//
// Why the winners are a FOREST that spans.  A CAS on parent[hi] that succeeds found hi still a root at the instant the
// atomic was resolved.  A root is the minimum of its set (parent[x] <= x always, and every hook puts the larger root under
// a smaller node), so lo < hi cannot be in hi's set — even where lo itself is stale and no root any more: it is a node of
// SOME other set.  Every win therefore merges two distinct sets, and each merge of two sets is one win: the winners are
// acyclic, at most n - 1 over a whole call (edges[] never overflows), and exactly (sets before) - (sets after) per class.
// unite_won returns only when a and b are in one set — by its own hook (true) or by someone else's (false) — so after a
// class's launch every row of the class has its end points joined: the sets are the components of all rows handled so far.
// Rows that repeat — mirror images, the block index's repeats, self-pairs (skipped) in a raw piece list — are harmless: a
// second CAS for a pair already joined cannot win, because its roots are equal and no CAS is tried.
//
// Why the winners are MINIMUM.  The host runs the classes one after another with a kernel boundary between only_dist = t
// and t + 1.  When class t + 1 starts, parent[] holds exactly the components at bound t (above), every hook visible.  A
// row of class t + 1 wins only if its end points are in different sets then or later, that is: not joined by any path of
// lighter edges.  That is Kruskal's rule with a concurrent inner loop; within one class every edge weighs the same, and any
// spanning forest of the class's contracted graph will do.  Uniting SEVERAL classes in one launch would break it: a heavy
// row could win a hook that a path of lighter rows, not yet handled, makes redundant — the forest would still span but
// would not be minimum, and level_ends[t] would come out too small for the light levels.
// Which of several rows of one class wins depends on arrival: the chosen edges of equal weight may differ from run to run.
// The numbers of edges per class and the partitions after every class do not.
//
// No flags, no spinning, no hand-off between workgroups: the only synchronisation is the atomics on parent[] and on the two
// running totals, and the kernel boundary.
#pragma once

#include "components.hip.h"

namespace smafa_sf {

__global__ void init_forest_kernel(uint32_t *__restrict__ parent, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = i;
}

// smafa_cc::unite, and whether this call's own CAS made the hook: find both roots; equal: joined by someone else, false;
// else CAS(parent[hi], hi, lo); won: true; lost (hi was hooked by someone else meanwhile): go on from the value the CAS
// returned, an ancestor of hi
__device__ __forceinline__ bool unite_won(uint32_t *parent, uint32_t a, uint32_t b) {
    uint32_t ra = smafa_cc::find_root(parent, a), rb = smafa_cc::find_root(parent, b);
    while (ra != rb) {
        const uint32_t hi = max(ra, rb), lo = min(ra, rb);
        const uint32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return true;
        ra = smafa_cc::find_root(parent, seen);
        rb = smafa_cc::find_root(parent, lo);
    }
    return false;
}

// The piece's list as join_filter_kernel receives it, and its rule: a row is kept iff position(query row) <
// pos_of[subject], which drops self-pairs, mirror images and the block index's repeats.  A kept row leaves as {a, b, dist}
// in subject numbers for kept[first + ...], one reservation per wave on ctl[0] (the kept total, exact at any capacity;
// zeroed by the host once per call); rows past cap are counted and not stored.  parent[] is not touched.
__global__ __launch_bounds__(256) void keep_pairs_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, smafa_hit *kept,
                                                         unsigned long long cap, unsigned long long *ctl) {
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
            if (keep) h.query = order[qpos];  // (another position than the subject's: another subject number)
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

// One weight class: the rows with dist == only_dist, all others pass by.  order != nullptr: a raw piece list, rows {record
// number of the query row in its span, subject number, dist} as link_rows_kernel receives them; order == nullptr: the kept
// list, rows {a, b, dist} in subject numbers (p0, S, R unused).  The early-out of link_rows_kernel comes first: equal parents
// are one set already, and no CAS of this row could win.  A lane that won writes its row, smaller number first, to
// edges[first + ...], one reservation per wave on *n_edges (the running edge total of the call: classes below this one have
// filled edges[0 .. *n_edges) when the launch starts).  cap = n - 1 is never reached (header); the compare keeps a wrong
// parent[] from writing past the caller's buffer.
__global__ __launch_bounds__(256) void span_edges_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order, uint32_t *parent,
                                                         uint32_t only_dist, smafa_hit *edges, unsigned long long cap,
                                                         unsigned long long *n_edges) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        const unsigned long long i = base + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool won = false;
        if (i < total) {
            h = list[i];
            if (h.dist == only_dist) {
                const uint32_t a = order ? order[p0 + (h.query % R) * S + h.query / R] : h.query, b = h.subject;
                if (a != b && smafa_cc::load_parent(parent, a) != smafa_cc::load_parent(parent, b)) won = unite_won(parent, a, b);
                h.query = min(a, b);
                h.subject = max(a, b);
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

// Bounds no two rows can exceed, after the class seq_len - 1: parent[] is final and read-only (the kernel boundary made every
// hook visible; plain loads).  Two rows in different sets now are at distance exactly seq_len — they differ in every column,
// or a lighter class had joined them — and row 0 is the root of its own set, so every other root r gets the edge
// (0, r, seq_len): a spanning TREE, n - 1 edges, as the components call says "one component" there.  level_ends[t] = n - 1
// for t = seq_len .. T - 1 is written here as well: it needs no count.
__global__ __launch_bounds__(256) void star_roots_kernel(const uint32_t *__restrict__ parent, uint32_t n, uint32_t seq_len,
                                                         smafa_hit *edges, unsigned long long cap,
                                                         unsigned long long *n_edges, unsigned long long *level_ends,
                                                         uint32_t T) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = i != 0u && i < n && parent[i] == i;
    const unsigned long long mask = __ballot(root);
    if (mask != 0ull) {
        unsigned long long first = 0;
        if ((threadIdx.x & 63u) == 0u) first = atomicAdd(n_edges, (unsigned long long)__builtin_popcountll(mask));
        first = smafa::shfl_u64(first, 0);
        const unsigned long long slot = first + smafa::lanes_below(mask);
        if (root && slot < cap) edges[slot] = smafa_hit{0u, i, seq_len};
    }
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)seq_len + i; t < T; t += stride) level_ends[t] = (unsigned long long)n - 1ull;
}

}  // namespace smafa_sf

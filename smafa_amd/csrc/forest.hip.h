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

// The loop body of keep_pairs_kernel and of smafa_mr::tally_keep_kernel, row i of a raw piece list under the exactly-once rule
// (piece.hip.h); the whole wave calls it, i < total or not.  A kept row leaves as {a, b, dist} in subject numbers for the kept
// list through piece::wave_append on ctl[0] (the kept total, exact at any capacity; zeroed by the host once per call); rows past
// cap are counted and not stored.  per_row(h) sees every kept row, stored or not.
template <class PerRow>
__device__ __forceinline__ void keep_row(const smafa_hit *__restrict__ list, unsigned long long total, unsigned long long i, uint32_t p0,
                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order, const uint32_t *__restrict__ pos_of,
                                         smafa_hit *kept, unsigned long long cap, unsigned long long *ctl, PerRow per_row) {
    smafa_hit h = {0, 0, 0};
    bool keep = false;
    if (i < total) {
        h = list[i];
        keep = piece::keep_once(h, p0, S, R, order, pos_of);
        if (keep) per_row(h);
    }
    const unsigned long long slot = piece::wave_append(keep, ctl);
    if (keep && slot < cap) kept[slot] = h;
}

struct NothingPerRow {
    __device__ __forceinline__ void operator()(const smafa_hit &) const {}
};

// keep_row and nothing else: parent[] is not touched
__global__ __launch_bounds__(256) void keep_pairs_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, smafa_hit *kept,
                                                         unsigned long long cap, unsigned long long *ctl) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;  // (uniform trip count per workgroup)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride)
        keep_row(list, total, base + threadIdx.x, p0, S, R, order, pos_of, kept, cap, ctl, NothingPerRow{});
}

// The loop body of span_edges_kernel and of smafa_mr::span_reach_kernel, row i of a list in either form (piece.hip.h: pair_of);
// the whole wave calls it, i < total or not.  One weight class, cls.t: all other rows pass by — cls.maybe(dist) before any
// gather, cls.is(dist, a, b) with the two subjects in hand.  Self-pairs are skipped, and the early-out of link_rows_kernel
// comes first: equal parents are one set already, and no CAS of this row could win.  A lane that won writes {min, max, cls.t}
// (a DistClass row carries t already: the store of the weight is for the classes whose weight is not the distance) through
// piece::wave_append on *n_edges (the running edge total of the call: classes below this one have filled edges[0 .. *n_edges)
// when the launch starts).  cap = n - 1 is never reached (header); the compare keeps a wrong parent[] from writing past the
// caller's buffer.
template <class Class>
__device__ __forceinline__ void span_row(const smafa_hit *__restrict__ list, unsigned long long total, unsigned long long i, uint32_t p0,
                                         uint32_t S, uint32_t R, const uint32_t *__restrict__ order, uint32_t *parent, smafa_hit *edges,
                                         unsigned long long cap, unsigned long long *n_edges, Class cls) {
    smafa_hit h = {0, 0, 0};
    bool won = false;
    if (i < total) {
        h = list[i];
        if (cls.maybe(h.dist)) {
            const uint32_t a = piece::pair_of(h, p0, S, R, order), b = h.subject;
            if (a != b && cls.is(h.dist, a, b) && smafa_cc::load_parent(parent, a) != smafa_cc::load_parent(parent, b))
                won = unite_won(parent, a, b);
            h.query = min(a, b);
            h.subject = max(a, b);
            h.dist = cls.t;
        }
    }
    const unsigned long long slot = piece::wave_append(won, n_edges);
    if (won && slot < cap) edges[slot] = h;
}

// the rows with dist == t
struct DistClass {
    uint32_t t;
    __device__ __forceinline__ bool maybe(uint32_t dist) const { return dist == t; }
    __device__ __forceinline__ bool is(uint32_t, uint32_t, uint32_t) const { return true; }
};

__global__ __launch_bounds__(256) void span_edges_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order, uint32_t *parent,
                                                         uint32_t only_dist, smafa_hit *edges, unsigned long long cap,
                                                         unsigned long long *n_edges) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;  // (uniform trip count per workgroup)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride)
        span_row(list, total, base + threadIdx.x, p0, S, R, order, parent, edges, cap, n_edges, DistClass{only_dist});
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
    const unsigned long long slot = piece::wave_append(root, n_edges);
    if (root && slot < cap) edges[slot] = smafa_hit{0u, i, seq_len};
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)seq_len + i; t < T; t += stride) level_ends[t] = (unsigned long long)n - 1ull;
}

}  // namespace smafa_sf

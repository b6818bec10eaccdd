// stable.hip.h — kernels of the STABLE CLUSTERS of a resident store (engine.hip: smafa_db_self_stable_launch): HDBSCAN's selection
// over the mutual-reachability forest of reach.hip.h, level by level.  The definition is include/smafa_amd.h's; in short: at
// level t a row is IN iff core[i] <= t, a component of the graph cut at weight t is BIG iff it holds min_cluster_size rows that
// are in, a big component with exactly one big component of level t - 1 inside it CONTINUES that one's cluster and every other big
// component STARTS one; a cluster's stability is the sum of its components' sizes over its levels, and a cluster is chosen iff
// its stability is at least the sum of the best of its children and no ancestor is chosen.
//
// The call works from the reach forest alone: at most n - 1 edges {a, b, w} ordered by w, and core[].  The levels are PLANES: plane
// t < seq_len is level t; where max_div >= seq_len the last plane, seq_len, stands for the levels seq_len .. max_div, which are all
// alike (one set, or no row in at all), and counts `mult` = max_div - seq_len + 1 times in a stability.  Per plane t, one launch each:
//   unite_class_kernel  per edge with w == t: smafa_cc::unite over parent[], which was fresh (parent[i] = i) before plane 0 and
//                       is never reset: behind the launch it holds the components of the graph cut at weight t
//   snapshot_kernel     per row: root[t][i] = the root of i = the smallest row of its set = lab_t[i]; a row that is in raises size[root]
//   census_kernel       per big component of plane t - 1: kids[root[t][it]]++
//   adopt_kernel        per big component of plane t - 1: where its component of plane t has one kid, that one inherits the running
//                       stability and the children's sum; else the cluster ends here: its best is added to the parent's children's
//                       sum and whether it won is flagged.  Per big component of plane t with kids != 1: a cluster starts.
// then excess_kernel ends the clusters of the last plane (the roots), choose_kernel runs once per plane from the last one down —
// a cluster's end is chosen iff it won and nothing above it is chosen, and the verdict is handed down its chain and to
// whatever ends under it — and assign_kernel walks every row up its planes: the first component that belongs to a chosen cluster
// gives joined[i], the last one of that chain labels[i].
//
// Why the class-by-class snapshots are exactly lab_t.  The forest's contract (reach.hip.h) is that the edges with w <= t are
// acyclic and connect exactly the graph cut at weight t.  unite_class_kernel of plane t returns from every edge of class t with
// its ends in one set (smafa_cc::unite), the kernel boundary makes every hook visible, and the classes below were united by
// the launches before: behind the launch parent[] holds the components of the cut at t and nothing else.  A root is the smallest
// row of its set (parent[x] <= x, the larger root goes under the smaller), so the root is lab_t[i] whatever the order of the
// hooks was: every output of this call is a function of the store, max_div, min_pts and min_cluster_size alone.
//
// Who writes what, launch by launch (no slot has two plain writers, or a plain writer and an atomic, in one launch):
//   size[cur], sum[cur]  zeroed on the stream in front of the plane; size by atomicAdd in snapshot_kernel, read from census on
//   kids[i]              zeroed by lane i in snapshot_kernel, raised by atomicAdd in census_kernel, read in adopt_kernel
//   run[cur][p]          kids[p] == 1: by the lane of p's one big child; else by lane p
//   sum[cur][p]          kids[p] == 1: by the lane of p's one big child; else by atomicAdd of the lanes of its big children
//   flag[t][x]           adopt_kernel of plane t (lane x), then adopt_kernel of plane t + 1 or excess_kernel (lane x: the end of a
//                        cluster), then choose_kernel of plane t (lane x; it reads flag[t + 1][..], final since the launch before)
// size, run and sum are kept for two planes only (cur = t & 1, the plane before in the other half).
// No flags to wait on, no spinning, no hand-off between workgroups, no inline assembly: the only synchronisation is the atomics
// named above and the kernel boundary.  Every load of parent[] inside the union is smafa_cc::load_parent.
#pragma once

#include "components.hip.h"

namespace smafa_st {

// flag[t][x], x a root of plane t
constexpr uint32_t kBig = 1u;      // the component holds min_cluster_size rows that are in
constexpr uint32_t kStart = 2u;    // a cluster starts here (kids != 1)
constexpr uint32_t kEnd = 4u;      // a cluster ends here (the component above has kids != 1, or this is the last plane)
constexpr uint32_t kWon = 8u;      // ... and its stability is at least the sum of the best of its children
constexpr uint32_t kChosen = 16u;  // the component belongs to a chosen cluster
constexpr uint32_t kClosed = 32u;  // the component's cluster or an ancestor of it is chosen: nothing under it can be

// One weight class of the forest's edges: edges[0 .. *n_edges) (the reach call's running edge total, final; never above cap =
// n - 1), a lane acts iff its edge weighs only_dist.
__global__ __launch_bounds__(256) void unite_class_kernel(const smafa_hit *__restrict__ edges, const unsigned long long *__restrict__ n_edges,
                                                          unsigned long long cap, uint32_t n, uint32_t only_dist, uint32_t *parent) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || i >= *n_edges) return;
    const smafa_hit h = edges[i];
    if (h.dist != only_dist || h.query >= n || h.subject >= n) return;  // (the compare keeps a wrong edge from reaching outside parent[])
    if (smafa_cc::load_parent(parent, h.query) != smafa_cc::load_parent(parent, h.subject)) smafa_cc::unite(parent, h.query, h.subject);
}

// Behind the class's launch the sets are final for this plane.  root[i] = lab_t[i], found with smafa_cc::find_root: its path
// halving only re-points a node at an ancestor, which no other lane's find can mind, and keeps the walks of the planes above
// short.  A row that is in at this plane counts at its root.
__global__ __launch_bounds__(256) void snapshot_kernel(uint32_t *parent, const uint32_t *__restrict__ core, uint32_t n, uint32_t t,
                                                       uint32_t *__restrict__ root, uint32_t *size, uint32_t *__restrict__ kids) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = smafa_cc::find_root(parent, i);
    root[i] = x;
    kids[i] = 0u;
    if (core[i] <= t) atomicAdd(size + x, 1u);  // (SMAFA_NONE, a sparse row, is above every plane)
}

// size_below[x] is 0 unless x was a root of the plane below with rows that are in: a big component there is a kid of the
// component it lies in now (which is big too: its rows stay in and together)
__global__ __launch_bounds__(256) void census_kernel(const uint32_t *__restrict__ size_below, const uint32_t *__restrict__ root, uint32_t n,
                                                     uint32_t min_size, uint32_t *kids) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n && size_below[x] >= min_size) atomicAdd(kids + root[x], 1u);
}

// Lane x, first as a big component of the plane below (below != 0: t > 0), then as a component of this plane; the two halves touch
// different slots (header).  run: the stability of the cluster so far; sum: the best of its children, added up.
__global__ __launch_bounds__(256) void adopt_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                    const uint32_t *__restrict__ size_below, const uint32_t *__restrict__ kids, uint32_t n,
                                                    uint32_t min_size, unsigned long long mult, uint32_t below,
                                                    const unsigned long long *__restrict__ run_below,
                                                    const unsigned long long *__restrict__ sum_below, unsigned long long *run,
                                                    unsigned long long *sum, uint32_t *flag_below, uint32_t *__restrict__ flag) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    if (below && size_below[x] >= min_size) {
        const uint32_t p = root[x];
        const unsigned long long mine = run_below[x], kin = sum_below[x];
        if (kids[p] == 1u) {
            run[p] = mine + (unsigned long long)size[p] * mult;
            sum[p] = kin;
        } else {
            atomicAdd(sum + p, max(mine, kin));
            flag_below[x] |= kEnd | (mine >= kin ? kWon : 0u);
        }
    }
    uint32_t f = 0u;
    if (size[x] >= min_size) {
        f = kBig;
        if (kids[x] != 1u) {
            f |= kStart;
            run[x] = (unsigned long long)size[x] * mult;
        }
    }
    flag[x] = f;
}

// the big components of the last plane end their clusters: the roots of the cluster tree
__global__ __launch_bounds__(256) void excess_kernel(const unsigned long long *__restrict__ run, const unsigned long long *__restrict__ sum,
                                                     uint32_t n, uint32_t *flag) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const uint32_t f = flag[x];
    if (f & kBig) flag[x] = f | kEnd | (run[x] >= sum[x] ? kWon : 0u);
}

// One plane, from the last one down.  `up` is the component of the plane above that this one lies in (root_above == nullptr: the
// last plane, nothing above).  An end: closed from above, or chosen if it won (a tie goes to the parent: kWon is >=).  No end: the
// component above is the same cluster's, and its verdict is this one's.  The chosen ends are counted, one atomicAdd per wave.
__global__ __launch_bounds__(256) void choose_kernel(const uint32_t *__restrict__ root_above, const uint32_t *__restrict__ flag_above,
                                                     uint32_t n, uint32_t *flag, unsigned long long *n_chosen) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    bool chosen = false;
    if (x < n) {
        uint32_t f = flag[x];
        if (f & kBig) {
            const uint32_t up = root_above ? flag_above[root_above[x]] : 0u;
            if (!(f & kEnd)) {
                f |= up & (kChosen | kClosed);
            } else if (up & kClosed) {
                f |= kClosed;
            } else if (f & kWon) {
                f |= kChosen | kClosed;
                chosen = true;
            }
            flag[x] = f;
        }
    }
    const unsigned long long mask = __ballot(chosen);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(n_chosen, (unsigned long long)__builtin_popcountll(mask));
}

// One lane per row, up its planes from the first at which it is in (root and flag plane-major, n entries a plane).  The first
// component that belongs to a chosen cluster: joined = that plane; the chain is followed while the component above is chosen too
// (it is the same cluster's: no ancestor of a chosen cluster is chosen), and its last root is the label.  None: noise.
__global__ __launch_bounds__(256) void assign_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ flag,
                                                     const uint32_t *__restrict__ core, uint32_t n, uint32_t planes,
                                                     uint32_t *__restrict__ labels, uint32_t *__restrict__ joined) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t label = SMAFA_NONE, since = SMAFA_NONE;
    for (uint32_t t = core[i]; t < planes; t++) {
        const uint32_t r = root[(size_t)t * n + i];
        if (!(flag[(size_t)t * n + r] & kChosen)) {
            if (label != SMAFA_NONE) break;
            continue;
        }
        if (label == SMAFA_NONE) since = t;
        label = r;
    }
    labels[i] = label;
    if (joined) joined[i] = since;
}

}  // namespace smafa_st

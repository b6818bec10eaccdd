// components.hip.h — kernels of the single-linkage components of a resident store (engine.hip:
// smafa_db_self_components_launch): labels[i] = the smallest subject number in i's connected component of the graph whose
// edges are the pairs within a bound.  The self-join's driver finds the pairs (join.hip.h, the scan kernels unchanged); the
// three kernels here consume each block's scratch list in place of join_filter_kernel — a concurrent union-find over
// parent[], one uint32 per subject, in a namespace of its own:
//   init_labels_kernel     parent[i] = i
//   link_rows_kernel       per row of a block's list: unite(subject number of the query row, subject number of the subject row)
//   flatten_labels_kernel  a launch of its own after the last block: labels[i] = root(i), representatives counted
//
// The union-find.  Hooking rule: the LARGER root goes under the SMALLER, by atomicCAS on the larger root's own slot, so
// parent[x] <= x holds at every instant: no cycles, and once every link has run a root is the minimum of its set — the
// label the call promises, whatever the order the rows arrived in.  Every write to parent[] after init_labels_kernel is
// an atomic (the CAS of a hook, the atomicMin of path halving) and only ever LOWERS a slot; a slot that has left x (the
// node was hooked) never returns to x.
//
// Visibility (which loads are atomic): workgroups of one link launch run on all XCDs, whose L2s are private, and race with
// each other's hooks.  Every load of parent[] inside link_rows_kernel is an agent-scope relaxed atomic load (load_parent:
// it bypasses the CU's L1, so a re-read in the find loop is not answered from a line the CU already holds).  That is for
// progress, not for correctness: a value that is out of date is still an ANCESTOR of the node in the same set (slots only
// go down the node's own chain of ancestors), so a find that follows one ends at a node of the right set, and whether that
// node is still a root is decided by the CAS alone, which compares with the slot's current value where the atomics are
// resolved.  A hook on a stale "root" lo merely hangs hi under a node that has a smaller ancestor by now — the sets are
// merged all the same.  flatten_labels_kernel is a later launch: the kernel boundary makes every hook visible, nothing
// writes parent[] any more, and its loads are plain.
//
// No flags, no spinning, no hand-off between workgroups: the only synchronisation is the atomics on parent[] and the
// kernel boundary.
#pragma once

#include "piece.hip.h"

namespace smafa_cc {

__global__ void init_labels_kernel(uint32_t *__restrict__ parent, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = i;
}

__device__ __forceinline__ uint32_t load_parent(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's set as this lane can see it, with path HALVING: every other node on the way is re-pointed at its
// grandparent (atomicMin: the grandparent is an ancestor no larger than the parent, and a slot another lane has lowered
// further meanwhile stays where it is).  Linking by index alone, without ranks, can build chains as long as a component;
// halving keeps later finds short.
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = load_parent(parent, x);
        if (p == x) return x;
        const uint32_t g = load_parent(parent, p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

// unite the sets of a and b: find both roots; equal: done; else CAS(parent[hi], hi, lo); lost (hi was hooked by someone
// else meanwhile): go on from the value the CAS returned, an ancestor of hi
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
    uint32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const uint32_t hi = max(ra, rb), lo = min(ra, rb);
        const uint32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        ra = find_root(parent, seen);
        rb = find_root(parent, lo);
    }
}

// A raw piece list (piece.hip.h), self-pairs, mirror images and (block index) repeats included — union is idempotent, so none
// of them needs filtering and neither pos_of[] nor the exactly-once rule is used.
// Early-out: one load of each parent; equal parents are one set already (in a dense family nearly every row).
__global__ __launch_bounds__(256) void link_rows_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                        uint32_t p0, uint32_t S, uint32_t R,
                                                        const uint32_t *__restrict__ order, uint32_t *parent) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const smafa_hit h = list[i];
        const uint32_t a = order[piece::piece_pos(h.query, p0, S, R)], b = h.subject;
        if (a == b) continue;
        if (load_parent(parent, a) == load_parent(parent, b)) continue;
        unite(parent, a, b);
    }
}

// After the last block, a launch of its own: parent[] is final and read-only here.  labels[i] = root of i = the smallest
// subject number of i's component; the representatives (labels[i] == i) are counted with one atomicAdd per wave.
__global__ __launch_bounds__(256) void flatten_labels_kernel(const uint32_t *__restrict__ parent, uint32_t n,
                                                             uint32_t *__restrict__ labels,
                                                             unsigned long long *n_components) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool rep = false;
    if (i < n) {
        uint32_t x = i, p = parent[x];
        while (p != x) {
            x = p;
            p = parent[x];
        }
        labels[i] = x;
        rep = x == i;
    }
    piece::wave_count(rep, n_components);  // the wave's first representative adds for all of them
}

}  // namespace smafa_cc

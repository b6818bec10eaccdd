// density.hip.h — kernels of the density clusters of a resident store (engine.hip: smafa_db_self_density_launch): DBSCAN
// over the store's own rows with eps = the bound and the Hamming distance of the scan kernels.  degree[i] = the number of
// OTHER subjects within the bound of subject i; i is a CORE row iff degree[i] + 1 >= min_pts; clusters are the connected
// components of the core rows under the core-core pairs within the bound, labelled by their smallest core subject number;
// a non-core row with a core row within the bound is a BORDER row and takes the label of its smallest-numbered core
// neighbour; every other row is noise (SMAFA_NONE).  The self-join's driver finds the pairs (join.hip.h, the scan kernels
// unchanged); the four kernels here are the fourth consumer of a finished piece's scratch list, next to join_filter_kernel
// (join.hip.h), link_rows_kernel (components.hip.h) and hook_levels_kernel (levels.hip.h), in a namespace of their own:
//   init_density_kernel     degree[i] = 0, parent[i] = i, attach[i] = NONE
//   count_keep_kernel       per row of a piece's list that the exactly-once rule keeps: degree[a]++, degree[b]++, and the row
//                           {a, b, dist} moves to the handle's KEPT PAIR LIST while that has room
//   link_cores_kernel       per row {a, b}: both core -> unite(a, b); one core -> attach[the other] = min(.., the core one)
//   flatten_density_kernel  a launch of its own after the last link: labels, degrees, {clusters, core rows, noise rows}
//
// Two phases, with a kernel boundary between them.  Whether a row is core is known only once EVERY pair has been counted,
// so no link can run while a count is still running: phase 1 is the whole join with count_keep_kernel per piece, phase 2
// links.  Phase 2 reads the kept pair list in one launch where that list held every kept row (one join), or is the join
// once more with link_cores_kernel as the piece consumer (two joins; engine.hip decides from the kept total).  A stale
// degree[] is therefore impossible: every load of degree[] in link_cores_kernel and flatten_density_kernel comes after the
// last count_keep_kernel has ended, nothing writes degree[] any more, and the loads are plain.
//
// What is atomic, and why the answer does not depend on the order the rows arrive in.
//   degree[]  atomicAdd only, in phase 1.  Integer addition commutes; the exactly-once rule (position(query row) <
//             pos_of[subject], as join_filter_kernel keeps rows) presents each unordered pair to exactly one lane of one
//             launch, whatever the pieces, the block index or the kernels that produced the lists, so the sums are exact —
//             also for the rows that find no room in the kept list, which are counted and not stored.
//   parent[]  the union-find of components.hip.h (smafa_cc::find_root / unite as they are: the larger root goes under the
//             smaller by atomicCAS, path halving by atomicMin, every load an agent-scope relaxed atomic load).  Unions are
//             made between two CORE rows only, so only core slots are ever written: a non-core slot stays a root of its
//             own from init_density_kernel to the end and no find ever follows it.  A root is the minimum of its set, and
//             every member of the set is core: the label is the smallest CORE subject number of the cluster.
//   attach[]  atomicMin only: a slot only ever goes DOWN, and ends as the minimum of the core neighbours offered to it,
//             in whatever order.  The core row's NUMBER is stored, not its label: the label is root(attach[i]), taken in
//             flatten_density_kernel when parent[] is final, so a border row within the bound of two clusters takes the
//             cluster of its smaller core neighbour, which need not be the cluster with the smaller label.
//   Union and atomicMin are idempotent, so link_cores_kernel is as correct on a raw piece list — self-pairs, mirror images
//   and (block index) repeats included — as on the kept list, where each pair appears once in one orientation: a row is
//   handled in both directions.
//   the kept list: piece::wave_append on the kept total.  The ORDER of the kept rows depends on arrival; nothing that reads
//   them does.
//
// No flags, no spinning, no hand-off between workgroups: the only synchronisation is the atomics above and the kernel
// boundary.
#pragma once

#include "components.hip.h"

namespace smafa_dn {

constexpr uint32_t kNone = 0xffffffffu;  // SMAFA_NONE

// d0 / one_set: the call at a bound no two rows can exceed (max_div >= seq_len) is answered without a scan — every degree
// is n - 1 and every row hangs under row 0; everywhere else d0 = 0 and every row is a set of its own.
__global__ void init_density_kernel(uint32_t *__restrict__ degree, uint32_t *__restrict__ parent,
                                    uint32_t *__restrict__ attach, uint32_t n, uint32_t d0, uint32_t one_set) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        degree[i] = d0;
        parent[i] = one_set ? 0u : i;
        attach[i] = kNone;
    }
}

__device__ __forceinline__ bool is_core(const uint32_t *__restrict__ degree, uint32_t i, uint32_t min_pts) {
    return degree[i] + 1u >= min_pts;  // (degree <= n - 1 < 2^32 - 1: no wrap)
}

// A raw piece list under the exactly-once rule (piece.hip.h).  Per kept row both degrees are raised, and the row leaves as
// {a, b, dist} in subject numbers for the kept list through piece::wave_append on ctl[0] (the kept total, exact at any
// capacity; zeroed by the host once per call); rows past cap are counted and not stored.
// ctl[1] becomes non-zero once some add has made a row core (the value an add returns is the row's degree before it): the
// host skips the link phase where no row is core.  One lane per wave writes it, and only while it still reads zero.
__global__ __launch_bounds__(256) void count_keep_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, uint32_t *degree,
                                                         uint32_t min_pts, smafa_hit *kept, unsigned long long cap,
                                                         unsigned long long *ctl) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        const unsigned long long i = base + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool keep = false, made_core = false;
        if (i < total) {
            h = list[i];
            keep = piece::keep_once(h, p0, S, R, order, pos_of);
            if (keep) {
                const uint32_t was_a = atomicAdd(degree + h.query, 1u), was_b = atomicAdd(degree + h.subject, 1u);
                made_core = max(was_a, was_b) + 2u >= min_pts;
            }
        }
        if (__ballot(made_core) != 0ull && lane == 0 && __hip_atomic_load(ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull)
            atomicOr(ctl + 1, 1ull);
        const unsigned long long slot = piece::wave_append(keep, ctl);
        if (keep && slot < cap) kept[slot] = h;
    }
}

// Phase 2, degree[] final (plain loads), over either list form (piece.hip.h: pair_of).  Both core: the early-out of
// link_rows_kernel on equal parents, then unite.  Exactly one
// core: the other row is offered the core row's number (a load first: a slot that is low enough already costs no atomic; an
// out-of-date value can only be too high, and then the atomicMin decides).  Neither: nothing.
__global__ __launch_bounds__(256) void link_cores_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ degree, uint32_t min_pts,
                                                         uint32_t *parent, uint32_t *attach) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const smafa_hit h = list[i];
        const uint32_t a = piece::pair_of(h, p0, S, R, order), b = h.subject;
        if (a == b) continue;
        const bool ca = is_core(degree, a, min_pts), cb = is_core(degree, b, min_pts);
        if (ca && cb) {
            if (smafa_cc::load_parent(parent, a) == smafa_cc::load_parent(parent, b)) continue;
            smafa_cc::unite(parent, a, b);
        } else if (ca || cb) {
            const uint32_t core = ca ? a : b, border = ca ? b : a;
            if (smafa_cc::load_parent(attach, border) > core) atomicMin(attach + border, core);
        }
    }
}

// After the last link, a launch of its own: parent[], degree[] and attach[] are final and read-only here.  A core row's
// label is its root (the smallest core number of its cluster); a border row's is the root of attach[i]; noise is NONE.
// counts[0..2] = {clusters (core rows that are their own root), core rows, noise rows}: ballot per wave, the four waves
// add in LDS, then one atomicAdd per workgroup and counter.
__global__ __launch_bounds__(256) void flatten_density_kernel(const uint32_t *__restrict__ parent,
                                                              const uint32_t *__restrict__ degree,
                                                              const uint32_t *__restrict__ attach, uint32_t n,
                                                              uint32_t min_pts, uint32_t *__restrict__ labels,
                                                              uint32_t *__restrict__ degrees,
                                                              unsigned long long *counts) {
    __shared__ uint32_t s_counts[3];
    if (threadIdx.x < 3u) s_counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool flags[3] = {false, false, false};  // representative of a cluster, core, noise
    if (i < n) {
        const uint32_t deg = degree[i];
        const bool core = deg + 1u >= min_pts;
        uint32_t x = core ? i : attach[i];
        if (x != kNone) {
            uint32_t p = parent[x];
            while (p != x) {
                x = p;
                p = parent[x];
            }
        }
        labels[i] = x;
        if (degrees) degrees[i] = deg;
        flags[0] = core && x == i;
        flags[1] = core;
        flags[2] = x == kNone;
    }
    for (int c = 0; c < 3; c++) {
        piece::wave_count(flags[c], &s_counts[c]);
    }
    __syncthreads();
    if (threadIdx.x < 3u && s_counts[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)s_counts[threadIdx.x]);
}

}  // namespace smafa_dn

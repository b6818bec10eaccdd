// peaks.hip.h — kernels of the abundance-peak clusters of a resident store (engine.hip: smafa_db_self_peaks_launch): the
// amplicon-denoising partition over the store's own rows.  With D = the bound and r <= D = the radius,
//   weight[i] = 1 + the number of OTHER subjects within r of subject i (r = 0: abundance; r = D: the ball count),
//   key(i)    = (weight[i], -i) in lexicographic order — the heavier row wins, ties go to the smaller subject number; no
//               two rows have equal keys,
//   parent[i] = the subject of greatest key among {i} and the subjects within D of i; parent[i] == i makes i a PEAK,
//   labels[i] = the peak reached from i along parent[].  The key strictly increases along every step, so parent[] is a
//               forest and every walk ends.
// The self-join's driver finds the pairs (join.hip.h, the scan kernels unchanged); the kernels here are the fifth consumer
// of a finished piece's scratch list, next to join_filter_kernel (join.hip.h), link_rows_kernel (components.hip.h),
// hook_levels_kernel (levels.hip.h) and count_keep_kernel (density.hip.h), in a namespace of their own:
//   init_peaks_kernel   mode 0: weight[i] = w0 (1, or n where every row is within r of every row); mode 1, a launch between
//                       the phases: best[i] = key(i)
//   weigh_keep_kernel   phase 1, per row of a piece's list that the exactly-once rule keeps: dist <= r raises both weights, and
//                       the row {a, b, dist} moves to the handle's KEPT PAIR LIST while that has room
//   climb_kernel        phase 2, per row {a, b}: the slot of the lower key is offered the higher key (atomicMax)
//   crown_kernel        only at a bound no two rows can exceed: the greatest key of the store, one slot
//   settle_kernel       parent[i] from best[i] (or the crown); labels = parents, weights, peaks counted
//   jump_kernel         pointer doubling in place on the labels, launched by the host until a round changes nothing
// With GIVEN weights (smafa_db_self_peaks_weighted_launch: the sizes of a store dereplicated elsewhere) one line changes — weight[i]
// = w_in[i] + the sum of w_in[j] over the OTHER subjects within r — and the first two kernels take the weights as an argument:
//   init_peaks_kernel   mode 2: weight[i] = w_in[i], and the sum of all w_in[] in one 8-byte total (one atomicAdd per wave)
//   weigh_keep_kernel   w_in != nullptr: w_in[b] and w_in[a] in place of the two ones
// The host checks that total against 2^32 - 1 before anything is weighed, so no weight can wrap; everything said below about
// weight[] holds unchanged (atomicAdd of integers only, each pair presented once).  Both arguments default to nullptr: the
// launches of the calls that count ones read as they did, and the kernels keep their names.
//
// Two phases, with a kernel boundary between them.  A key is known only once EVERY pair has been weighed, so no climb can
// run while a weigh is still running: phase 1 is the whole join with weigh_keep_kernel per piece, phase 2 climbs.  Phase 2
// reads the kept pair list in one launch where that list held every kept row (one join), or is the join once more with
// climb_kernel as the piece consumer (two joins; engine.hip decides from the kept total).  Every load of weight[] in
// init_peaks_kernel (mode 1), climb_kernel, crown_kernel and settle_kernel comes after the last weigh_keep_kernel has ended,
// nothing writes weight[] any more, and the loads are plain.
//
// What is atomic, and why the answer does not depend on the order the rows arrive in.
//   weight[]  atomicAdd only, in phase 1.  Integer addition commutes; the exactly-once rule (position(query row) <
//             pos_of[subject], as join_filter_kernel keeps rows) presents each unordered pair to exactly one lane of one
//             launch, whatever the pieces, the block index or the kernels that produced the lists, so the sums are exact —
//             also for the rows that find no room in the kept list, which are counted and not stored.
//   best[]    8 B per subject, (weight << 32) | (0xFFFFFFFF - number): comparing two slots as integers compares two keys.
//             atomicMax only, in phase 2: a slot only ever goes UP, from the row's own key to the maximum of the keys
//             offered to it, in whatever order.  Only the higher key of a pair is offered, and only to the slot of the lower,
//             so a slot ends as the greatest key among the row and its neighbours within D: the definition of parent[].  A
//             relaxed agent-scope load comes first — a slot that is high enough already costs no atomic; an out-of-date
//             value can only be too low, and then the atomicMax decides.  atomicMax is idempotent, so climb_kernel is as
//             correct on a raw piece list — self-pairs, mirror images and (block index) repeats included — as on the kept
//             list, where each pair appears once in one orientation.
//   the kept list: piece::block_append on the kept total, ONE reservation per workgroup and loop iteration.  The ORDER of
//             the kept rows depends on arrival; nothing that reads them does.
//   the crown one slot, atomicMax of every key, one atomic per wave after a reduction across the lanes: the maximum of a set.
//   labels[]  jump_kernel: slot i is written by thread i alone, with an ancestor of i in parent[]'s forest — the value it
//             read at lab[lab[i]].  Whatever a racing thread reads in a slot is therefore an ancestor of that slot's row, old
//             or new, and a jump over it still lands on an ancestor: the slots only ever move towards their root.  A round
//             that changes nothing read every slot unchanged, so lab[lab[i]] == lab[i] for every i: every label is a root.
//             In-place jumping at least halves the longest remaining path per round, so a forest of < 2^32 rows is flat after
//             32 rounds and the 33rd changes nothing.  Loads and stores are relaxed agent-scope atomics (whole words, no
//             stale cache line); the one word the host reads is `changed`, stored by one lane of every wave that moved a slot.
//
// No flags between workgroups other than that word, no spinning, no hand-off: the only synchronisation is the atomics
// above and the kernel boundary.
#pragma once

#include "components.hip.h"

namespace smafa_pk {

constexpr uint32_t kNone = 0xffffffffu;  // SMAFA_NONE

__device__ __forceinline__ unsigned long long key_of(uint32_t weight, uint32_t i) {
    return ((unsigned long long)weight << 32) | (unsigned long long)(kNone - i);
}

// mode 0, in front of the join: weight[i] = w0.  mode 1, between the phases: best[i] = the row's own key (weight[] final).
// mode 2, in front of the join of a call with given weights: weight[i] = w_in[i], and *total (zeroed by the host) += their sum,
// reduced across the wave first — every lane of a wave reaches the reduction.
__global__ __launch_bounds__(256) void init_peaks_kernel(unsigned long long *__restrict__ best, uint32_t *__restrict__ weight,
                                                         uint32_t n, uint32_t w0, uint32_t mode,
                                                         const uint32_t *__restrict__ w_in = nullptr, unsigned long long *total = nullptr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 2u) {
        uint32_t w = 0;
        if (i < n) weight[i] = w = w_in[i];
        unsigned long long sum = w;
        for (int off = 32; off > 0; off >>= 1) sum += smafa::shfl_u64(sum, (int)((threadIdx.x & 63u) ^ (uint32_t)off));
        if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(total, sum);
        return;
    }
    if (i < n) {
        if (mode == 0u)
            weight[i] = w0;
        else
            best[i] = key_of(weight[i], i);
    }
}

// A raw piece list under the exactly-once rule (piece.hip.h).  A kept row within the radius raises both weights; EVERY kept
// row leaves as {a, b, dist} in subject numbers for the kept list through piece::block_append; with w_in the two weights are
// raised by the OTHER row's given weight instead of 1; rows past cap are counted in
// ctl[0] (the kept total, exact at any capacity; zeroed by the host once per call) and not stored.  The trip count of the
// loop is uniform per workgroup, so the two barriers of an append are met by all four waves.
__global__ __launch_bounds__(256) void weigh_keep_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                         uint32_t p0, uint32_t S, uint32_t R,
                                                         const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ pos_of, uint32_t *weight,
                                                         uint32_t radius, smafa_hit *kept, unsigned long long cap,
                                                         unsigned long long *ctl, const uint32_t *__restrict__ w_in = nullptr) {
    __shared__ uint32_t s_wave[2][4];
    __shared__ unsigned long long s_first[2];
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    uint32_t set = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride, set ^= 1u) {
        const unsigned long long i = base + threadIdx.x;
        smafa_hit h = {0, 0, 0};
        bool keep = false;
        if (i < total) {
            h = list[i];
            keep = piece::keep_once(h, p0, S, R, order, pos_of);
            if (keep && h.dist <= radius) {
                atomicAdd(weight + h.query, w_in ? w_in[h.subject] : 1u);
                atomicAdd(weight + h.subject, w_in ? w_in[h.query] : 1u);
            }
        }
        const unsigned long long slot = piece::block_append(keep, ctl, 1u, s_wave, s_first, set);
        if (keep && slot < cap) kept[slot] = h;
    }
}

// Phase 2, weight[] final (plain loads), over either list form (piece.hip.h: pair_of).  The row of the lower key is offered
// the higher key.
__global__ __launch_bounds__(256) void climb_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                    uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                    const uint32_t *__restrict__ weight, unsigned long long *best) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const smafa_hit h = list[i];
        const uint32_t a = piece::pair_of(h, p0, S, R, order), b = h.subject;
        if (a == b) continue;
        const unsigned long long ka = key_of(weight[a], a), kb = key_of(weight[b], b);
        const uint32_t lower = ka < kb ? a : b;
        const unsigned long long higher = ka < kb ? kb : ka;
        if (__hip_atomic_load(best + lower, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < higher) atomicMax(best + lower, higher);
    }
}

// max_div >= seq_len: every row is within the bound of every row, and every parent is the row of greatest key.  *crown is
// zeroed by the host; a key is never zero (its low word is 0xFFFFFFFF - i, i < n <= 2^32 - 1).
__global__ __launch_bounds__(256) void crown_kernel(const uint32_t *__restrict__ weight, uint32_t n, unsigned long long *crown) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long k = i < n ? key_of(weight[i], i) : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = smafa::shfl_u64(k, (int)((threadIdx.x & 63u) ^ (uint32_t)off));
        k = o > k ? o : k;
    }
    if ((threadIdx.x & 63u) == 0u && k) atomicMax(crown, k);
}

// After the last climb, a launch of its own: best[] and weight[] are final and read-only here.  crown != nullptr: every
// parent is the crown's row.  labels[i] = parent[i], for jump_kernel to flatten; the peaks (parent[i] == i) are counted by
// ballot per wave, the four waves add in LDS, then one atomicAdd per workgroup.
__global__ __launch_bounds__(256) void settle_kernel(const unsigned long long *__restrict__ best,
                                                     const uint32_t *__restrict__ weight, uint32_t n,
                                                     const unsigned long long *__restrict__ crown,
                                                     uint32_t *__restrict__ labels, uint32_t *__restrict__ parents,
                                                     uint32_t *__restrict__ weights, unsigned long long *n_peaks) {
    __shared__ uint32_t s_peaks;
    if (threadIdx.x == 0u) s_peaks = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool peak = false;
    if (i < n) {
        const uint32_t parent = kNone - (uint32_t)(crown ? *crown : best[i]);
        labels[i] = parent;
        if (parents) parents[i] = parent;
        if (weights) weights[i] = weight[i];
        peak = parent == i;
    }
    piece::wave_count(peak, &s_peaks);
    __syncthreads();
    if (threadIdx.x == 0u && s_peaks) atomicAdd(n_peaks, (unsigned long long)s_peaks);
}

// One round of pointer doubling in place (header: why any value read is an ancestor).  No thread ever walks to a root.
__global__ __launch_bounds__(256) void jump_kernel(uint32_t *lab, uint32_t n, uint32_t *changed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const uint32_t u = __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t uu = __hip_atomic_load(lab + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (uu != u) {
            __hip_atomic_store(lab + i, uu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            moved = true;
        }
    }
    if (piece::wave_first(moved)) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace smafa_pk

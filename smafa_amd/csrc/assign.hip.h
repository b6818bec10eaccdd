// assign.hip.h — kernels of the ABUNDANCE TABLE of a resident store (engine.hip: smafa_db_assign_launch): the reads of a resident
// query set assigned to their nearest subject within a bound and counted per (group, sample).  The definition is
// include/smafa_amd.h's; in short: best[q] = min over the subjects within the bound of (dist << 32 | subject) — the smallest
// distance, a tie to the smaller subject number —, a read's group is the value the caller's table holds for that subject
// (SMAFA_NONE for a read with no subject), and the table has one entry {group, sample, sum of weights} per pair that holds a read
// of weight > 0, ordered by (group, sample).
// The kernels live in `assign::`, not in a `smafa_xx::` namespace: the censuses of tests/ pin every namespace that begins with
// `smafa` to the kernels it holds today.
//
//   init_kernel    best[q] = all ones for the m reads, subject_counts[i] = 0 for the n subjects (where wanted), totals[0 .. 3] = 0.
//   best_kernel    per row of a span's list (the scan's rows at each read's minimum distance — but nothing here relies on
//                  that): one lane per row, the rows of one read that sit side by side in the wave are reduced to their
//                  minimum by a segmented scan, and the last lane of each such run does ONE 64-bit atomicMin into best[query].
//   bin_kernel     per read: best[q] unpacked into subject[q] and dist[q] (where wanted), the group looked up, the sort key
//                  group << sample_bits | sample and the value weight written; the weight added to subject_counts[subject]
//                  (where wanted) and to the assigned or unassigned total (summed over the wave first: one atomic per wave and
//                  total).  A read whose sample number is not below n_samples is counted in totals[3] and takes part in nothing
//                  else; it and every read of weight 0 get weight 0 and the DEAD key, all ones over the key's bits.
//                  sample_bits holds n_samples itself, not n_samples - 1, so that no live key is all ones: the dead reads sort
//                  behind every live one, and the table needs no second look at the weights.
//   (hipCUB radix sort of the (key, weight) pairs over 32 + sample_bits bits)
//   heads_kernel   per sorted element: mark[i] = 1 where a run of equal LIVE keys begins.  An exclusive sum over mark[0 .. m]
//                  gives every head its entry number and, at [m], the number of entries.
//   fold_kernel    per sorted live element: its entry number e = sum[i] + mark[i] - 1.  Lanes that hold the same e sit side by
//                  side; a segmented scan adds their weights and the last lane of each run in the wave does ONE 64-bit atomicAdd
//                  into entries[e].count — a run of a million reads costs one atomic per wave it crosses (m / 64), and no thread
//                  walks it.  The heads also write {group, sample} of their entry.  Entries at or above cap are not
//                  touched; the lane of the last element publishes the number of entries in totals[0].
//
// Everything is integer arithmetic on atomics that commute (minimum, addition): the bytes do not depend on the order in which
// rows, reads or waves arrive.  No flags, no spinning, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smafa_amd.h"

namespace assign {

typedef unsigned long long u64;

__device__ __forceinline__ u64 shfl_up_u64(u64 v, uint32_t delta) {
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), delta, 64);
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, delta, 64);
    return ((u64)hi << 32) | lo;
}

// Lanes that hold the same `id` side by side form a run.  first: the lane at which this lane's run begins; returns whether this
// lane is the last of its run in the wave.  All 64 lanes call it.
__device__ __forceinline__ bool run_of(uint32_t id, uint32_t lane, uint32_t *first) {
    const uint32_t before = (uint32_t)__shfl_up((int)id, 1u, 64);
    const u64 begins = __ballot(lane == 0u || before != id);  // (bit 0 is always set)
    *first = 63u - (uint32_t)__builtin_clzll(begins & (~0ull >> (63u - lane)));
    return lane == 63u || ((begins >> (lane + 1u)) & 1ull);
}

// the inclusive scan of `v` under `op` inside every run: the last lane of a run ends up with the run's result
template <class Op>
__device__ __forceinline__ u64 run_scan(u64 v, uint32_t lane, uint32_t first, Op op) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const u64 other = shfl_up_u64(v, d);
        if (lane >= first + d) v = op(v, other);
    }
    return v;
}

// the sum of `v` over the wave's 64 lanes, in every lane
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    return v;
}

// the key of a read that takes no part in the table: all ones over the key's 32 + sample_bits bits
__device__ __forceinline__ u64 dead_key(uint32_t sample_bits) { return sample_bits >= 32u ? ~0ull : (1ull << (32u + sample_bits)) - 1ull; }

__global__ __launch_bounds__(256) void init_kernel(u64 *__restrict__ best, uint64_t m, u64 *__restrict__ subject_counts, uint64_t n,
                                                   u64 *__restrict__ totals) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < m; i += stride) best[i] = ~0ull;
    if (subject_counts)
        for (uint64_t i = t; i < n; i += stride) subject_counts[i] = 0ull;
    if (t < 4u) totals[t] = 0ull;
}

// rows[0 .. count): the list of one span; every row's query is below m
__global__ __launch_bounds__(256) void best_kernel(const smafa_hit *__restrict__ rows, u64 count, uint32_t m, u64 *best) {
    const uint32_t lane = threadIdx.x & 63u;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < count; base += stride) {  // (a uniform trip count per workgroup)
        const u64 i = base + threadIdx.x;
        const bool live = i < count;
        uint32_t q = SMAFA_NONE;
        u64 mine = ~0ull;
        if (live) {
            const smafa_hit h = rows[i];
            q = h.query;
            mine = ((u64)h.dist << 32) | h.subject;
        }
        uint32_t first;
        const bool last = run_of(q, lane, &first);
        mine = run_scan(mine, lane, first, [](u64 a, u64 b) { return a < b ? a : b; });
        if (live && last && q < m) atomicMin(best + q, mine);
    }
}

// group_of: nullptr — a subject's group is its own number.  samples: nullptr — sample 0.  weights: nullptr — weight 1.
// subject, dist, subject_counts: nullptr where not wanted.  totals[1]: assigned weight, [2]: unassigned weight, [3]: reads whose
// sample number is out of range.
__global__ __launch_bounds__(256) void bin_kernel(const u64 *__restrict__ best, uint32_t m, const uint32_t *__restrict__ group_of,
                                                  const uint32_t *__restrict__ samples, uint32_t n_samples, uint32_t sample_bits,
                                                  const uint32_t *__restrict__ weights, uint32_t *__restrict__ subject,
                                                  uint32_t *__restrict__ dist, u64 *subject_counts, u64 *__restrict__ keys,
                                                  uint32_t *__restrict__ values, u64 *totals) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = q < m;
    u64 in = 0ull, out = 0ull;
    bool stray = false;
    if (live) {
        const u64 b = best[q];
        const bool found = b != ~0ull;
        const uint32_t s = found ? (uint32_t)b : SMAFA_NONE, d = found ? (uint32_t)(b >> 32) : SMAFA_NONE;
        if (subject) subject[q] = s;
        if (dist) dist[q] = d;
        const uint32_t sample = samples ? samples[q] : 0u;
        stray = sample >= n_samples;
        const uint32_t w = stray ? 0u : weights ? weights[q] : 1u;
        const uint32_t g = !found ? SMAFA_NONE : group_of ? group_of[s] : s;
        const u64 dead = dead_key(sample_bits);
        keys[q] = w ? ((u64)g << sample_bits) | sample : dead;
        values[q] = w;
        if (found) in = w;
        else out = w;
        if (found && w && subject_counts) atomicAdd(subject_counts + s, (u64)w);
    }
    // the three totals: summed over the wave, one atomic each
    const u64 strays = __ballot(stray);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // (wave_sum's steps for both at once: two calls of it schedule differently)
        in += ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(in >> 32), off, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)in, off, 64);
        out += ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(out >> 32), off, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)out, off, 64);
    }
    if (lane == 0u) {
        if (in) atomicAdd(totals + 1, in);
        if (out) atomicAdd(totals + 2, out);
        if (strays) atomicAdd(totals + 3, (u64)__builtin_popcountll(strays));
    }
}

// keys[0 .. m): sorted; mark[0 .. m]: mark[m] = 0
__global__ __launch_bounds__(256) void heads_kernel(const u64 *__restrict__ keys, uint32_t m, uint32_t sample_bits, uint32_t *__restrict__ mark) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const u64 dead = dead_key(sample_bits);
    mark[i] = i < m && keys[i] != dead && (i == 0u || keys[i - 1u] != keys[i]) ? 1u : 0u;
}

// sum[0 .. m]: the exclusive sum of mark[]; entries[0 .. cap): their counts zero on entry
__global__ __launch_bounds__(256) void fold_kernel(const u64 *__restrict__ keys, const uint32_t *__restrict__ values, const uint32_t *__restrict__ mark,
                                                   const uint32_t *__restrict__ sum, uint32_t m, uint32_t sample_bits, smafa_table_entry *entries,
                                                   u64 cap, u64 *__restrict__ totals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const u64 dead = dead_key(sample_bits);
    uint32_t e = SMAFA_NONE;  // (the dead tail and the lanes past the end: one run that adds nothing)
    u64 w = 0ull;
    bool head = false;
    u64 key = dead;
    if (i < m) {
        key = keys[i];
        if (key != dead) {
            head = mark[i] != 0u;
            e = sum[i] + (head ? 1u : 0u) - 1u;
            w = values[i];
        }
        if (i + 1u == m) totals[0] = sum[m];
    }
    uint32_t first;
    const bool last = run_of(e, lane, &first);
    w = run_scan(w, lane, first, [](u64 a, u64 b) { return a + b; });
    if (e == SMAFA_NONE || e >= cap) return;
    if (head) {
        entries[e].label = (uint32_t)(key >> sample_bits);
        entries[e].sample = (uint32_t)(key & ((1ull << sample_bits) - 1ull));
    }
    if (last) atomicAdd(reinterpret_cast<u64 *>(&entries[e].count), w);
}

}  // namespace assign

// classify.hip.h — kernels of the LCA CLASSIFICATION of a resident query set (engine.hip: smafa_db_classify_launch): every read
// given the lowest common ancestor of the lineages of its best hits, and counted per (taxon, sample).  The definition is
// include/smafa_amd.h's; in short: best[q] = min over the subjects within the bound of (dist << 32 | subject), as the abundance
// table has it — its subject is the read's ANCHOR —, B(q) = the subjects within best's distance + slack, depth[q] = the minimum
// over B(q) of the number of leading ranks at which the subject's lineage row equals the anchor's, ties[q] = |B(q)|, and the
// read's taxon is the anchor's id at rank depth - 1 (SMAFA_TAXON_ROOT at depth 0, SMAFA_NONE without an anchor).  On a tree the
// minimum of the common prefixes with ONE member is the depth of the LCA of all: no per-rank state, one integer per read.
// The kernels live in `classify::`, not in a `smafa_xx::` namespace.  The 64-bit minimum per read, the heads and
// the segmented sum are assign::best_kernel, assign::heads_kernel and assign::fold_kernel, launched as they are.
//
//   start_kernel   best[q] = all ones, depth[q] = R, ties[q] = 0 for the m reads, totals[0 .. 5] = 0.
//   agree_kernel   per row of a span's list, behind assign::best_kernel over the same list (a read's rows all lie in one span's
//                  list, so best[q] is final): one lane per row.  The row is a MEMBER iff dist <= best's distance + slack; a
//                  member's value is its common prefix with the anchor's row, in whole ranks.  The rows of one read that sit
//                  side by side in the wave are reduced by assign::run_scan — the minimum of the prefixes and the number of
//                  members, packed into one 64-bit value — and the last lane of each run does ONE atomicMin on depth[q] and ONE
//                  atomicAdd on ties[q].
//   key_kernel     per read: subject, dist, taxon, depth and ties written (where wanted), the sort key taxon << sample_bits |
//                  sample and the value weight written as assign::bin_kernel writes them (the same dead key), the totals [1] ..
//                  [5] summed over the wave first: one atomic per wave and total.
//
// Integer minimum and addition only: the bytes do not depend on the order in which rows, reads or waves arrive.  No flags, no
// spinning, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smafa_amd.h"
#include "assign.hip.h"

namespace classify {

typedef assign::u64 u64;

constexpr uint32_t kMaxRanks = 16;  // R of the contract: a lineage row is at most 64 B

__global__ __launch_bounds__(256) void start_kernel(u64 *__restrict__ best, uint32_t *__restrict__ depth, uint32_t *__restrict__ ties, uint64_t m,
                                                    uint32_t n_ranks, u64 *__restrict__ totals) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < m; i += stride) {
        best[i] = ~0ull;
        depth[i] = n_ranks;
        ties[i] = 0u;
    }
    if (t < 6u) totals[t] = 0ull;
}

// The number of leading ranks at which rows a and s of lineage[][n_ranks] hold the same id, SMAFA_NONE ending both.  The ranks go
// four at a time: the eight loads of a step are independent of each other (one round trip to memory, not one per rank), and a lane
// whose rows have parted asks for no further step.  Rows of 7 ranks are not 16-byte aligned: dword loads.  The index is clamped
// to the row, so that every load of a step is issued whatever n_ranks is.
__device__ __forceinline__ uint32_t common_ranks(const uint32_t *__restrict__ lineage, uint32_t n_ranks, uint32_t a, uint32_t s) {
    const uint32_t *const ra = lineage + (size_t)a * n_ranks, *const rs = lineage + (size_t)s * n_ranks;
    uint32_t cp = 0;
    for (uint32_t r0 = 0; r0 < n_ranks; r0 += 4u) {
        uint32_t va[4], vs[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t r = r0 + k < n_ranks ? r0 + k : n_ranks - 1u;
            va[k] = ra[r];
            vs[k] = rs[r];
        }
        bool same = true;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            same = same && r0 + k < n_ranks && va[k] == vs[k] && va[k] != SMAFA_NONE;
            cp += same ? 1u : 0u;
        }
        if (!same) break;
    }
    return cp;
}

// rows[0 .. count): the list of one span, behind assign::best_kernel over the same list; lineage holds n rows.  A row whose query
// is not below m, whose subject is not below n or whose read has no best[] yet (none of which the call produces) is no member.
__global__ __launch_bounds__(256) void agree_kernel(const smafa_hit *__restrict__ rows, u64 count, uint32_t m, const u64 *__restrict__ best,
                                                    uint32_t slack, const uint32_t *__restrict__ lineage, uint32_t n, uint32_t n_ranks,
                                                    uint32_t *depth, uint32_t *ties) {
    const uint32_t lane = threadIdx.x & 63u;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < count; base += stride) {  // (a uniform trip count per workgroup)
        const u64 i = base + threadIdx.x;
        uint32_t q = SMAFA_NONE;
        u64 mine = (u64)SMAFA_NONE << 32;  // (prefix, members): no member, and a prefix that lowers nothing
        if (i < count) {
            const smafa_hit h = rows[i];
            if (h.query < m && h.subject < n) {
                q = h.query;
                const u64 b = best[q];
                if (b != ~0ull && (u64)h.dist <= (b >> 32) + slack) mine = ((u64)common_ranks(lineage, n_ranks, (uint32_t)b, h.subject) << 32) | 1ull;
            }
        }
        uint32_t first;
        const bool last = assign::run_of(q, lane, &first);
        mine = assign::run_scan(mine, lane, first, [](u64 a, u64 b) {
            const u64 low = (a >> 32) < (b >> 32) ? (a >> 32) : (b >> 32);
            return (low << 32) | (uint32_t)((uint32_t)a + (uint32_t)b);
        });
        if (last && q != SMAFA_NONE && (uint32_t)mine) {
            atomicMin(depth + q, (uint32_t)(mine >> 32));
            atomicAdd(ties + q, (uint32_t)mine);
        }
    }
}

// samples: nullptr — sample 0.  weights: nullptr — weight 1.  subject, dist, taxon, depth_out, ties_out: nullptr where not wanted.
// totals[1]: assigned weight, [2]: unassigned weight, [3]: reads whose sample number is out of range, [4]: weight on the root,
// [5]: reads (of a sample in range) with more than one member.
__global__ __launch_bounds__(256) void key_kernel(const u64 *__restrict__ best, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ ties,
                                                  uint32_t m, const uint32_t *__restrict__ lineage, uint32_t n_ranks,
                                                  const uint32_t *__restrict__ samples, uint32_t n_samples, uint32_t sample_bits,
                                                  const uint32_t *__restrict__ weights, uint32_t *__restrict__ subject, uint32_t *__restrict__ dist,
                                                  uint32_t *__restrict__ taxon, uint32_t *__restrict__ depth_out, uint32_t *__restrict__ ties_out,
                                                  u64 *__restrict__ keys, uint32_t *__restrict__ values, u64 *totals) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    u64 in = 0ull, out = 0ull, root = 0ull;
    bool stray = false, tied = false;
    if (q < m) {
        const u64 b = best[q];
        const bool found = b != ~0ull;
        const uint32_t s = found ? (uint32_t)b : SMAFA_NONE, d = found ? (uint32_t)(b >> 32) : SMAFA_NONE;
        const uint32_t deep = found ? depth[q] : SMAFA_NONE, t = found ? ties[q] : 0u;
        const uint32_t x = !found ? SMAFA_NONE : deep ? lineage[(size_t)s * n_ranks + deep - 1u] : SMAFA_TAXON_ROOT;
        if (subject) subject[q] = s;
        if (dist) dist[q] = d;
        if (taxon) taxon[q] = x;
        if (depth_out) depth_out[q] = deep;
        if (ties_out) ties_out[q] = t;
        const uint32_t sample = samples ? samples[q] : 0u;
        stray = sample >= n_samples;
        const uint32_t w = stray ? 0u : weights ? weights[q] : 1u;
        const u64 dead = assign::dead_key(sample_bits);
        keys[q] = w ? ((u64)x << sample_bits) | sample : dead;
        values[q] = w;
        if (found) in = w;
        else out = w;
        if (found && !deep) root = w;
        tied = !stray && t > 1u;
    }
    // the five totals: summed over the wave, one atomic each
    const u64 strays = __ballot(stray), many = __ballot(tied);
    in = assign::wave_sum(in), out = assign::wave_sum(out), root = assign::wave_sum(root);
    if (lane == 0u) {
        if (in) atomicAdd(totals + 1, in);
        if (out) atomicAdd(totals + 2, out);
        if (strays) atomicAdd(totals + 3, (u64)__builtin_popcountll(strays));
        if (root) atomicAdd(totals + 4, root);
        if (many) atomicAdd(totals + 5, (u64)__builtin_popcountll(many));
    }
}

}  // namespace classify

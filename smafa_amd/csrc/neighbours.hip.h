// neighbours.hip.h — kernels of the neighbour lists of a resident store (engine.hip: smafa_db_self_neighbours_launch): the
// self-join's graph in the form graph tools take, row offsets plus per row its neighbours ordered by (distance, number),
// optionally cut to the k nearest.  With D = the bound,
//   N(i)       = { j != i : distance(i, j) <= D } ordered by (distance, j) ascending,
//   list(i)    = the first min(|N(i)|, k) entries of N(i),
//   offsets[i] = the start of list(i) in neighbours[] / dists[]; offsets[n] = the number of entries.
// The self-join's driver finds the pairs (join.hip.h, the scan kernels unchanged); the kernels here are the sixth consumer
// of a finished piece's scratch list and what runs behind the join, in a namespace of their own:
//   mirror_pack_kernel   per row of a piece's list that the exactly-once rule keeps, {a, b, d}: the two ENTRIES (a; d; b)
//                        and (b; d; a) are appended to the handle's entry list
//   row_bounds_kernel    behind the sort of the entry list by (row, dist, neighbour): lower[i] = the first sorted entry of
//                        a row >= i, one binary search per ROW (lower[n] = the number of entries)
//   cut_degrees_kernel   only with a cut: cut[i] = min(lower[i + 1] - lower[i], k); an exclusive sum turns them into offsets
//   emit_kernel          per sorted entry: rank = its index - lower[row]; rank < k goes to neighbours / dists at
//                        offsets[row] + rank
//
// An entry is 8 bytes.  Where (row, dist) fit 32 bits (engine.h: neighbour_key_rule) it is the whole sort key,
//   row << (32 + dist_bits) | dist << 32 | neighbour,
// and one radix sort of the keys orders the list.  Otherwise the entry is dist << 32 | neighbour with the row in a second,
// 4-byte list beside it, and two stable sorts — by the entry carrying the row, then by the row carrying the entry — give the
// same order.  row_bounds_kernel and emit_kernel read either form (rows == nullptr: the first).
//
// Why one global sort and no per-row cursors: the degrees are unknown until the join has ended, so cursors would need a
// counting join in front of the filling one or a second pass over a kept list, and the order within a row would still need
// a sort per row.  The sort is the library's radix sort; everything around it is a map over rows or over entries.
//
// What is atomic: the entry total alone, through piece::block_append with two entries per kept row: ONE reservation per
// workgroup and loop iteration.  The exactly-once rule presents each unordered pair to exactly one lane of one
// launch, so the list holds each directed pair once; its ORDER depends on arrival, and the sort — whose keys are all
// distinct — removes that.  No flags between workgroups, no spinning: the only synchronisation is that atomic and the
// kernel boundary.
#pragma once

#include "peaks.hip.h"

namespace smafa_nb {

// A raw piece list under the exactly-once rule (piece.hip.h).  Every kept row {a, b, d} leaves as two entries at the slot
// piece::block_append gives it and the one behind:
// shift != 0: (a << shift | d << 32 | b) and (b << shift | d << 32 | a); shift == 0: (d << 32 | b) with rows[] = a, and
// (d << 32 | a) with rows[] = b.  *total (zeroed by the host once per call) counts every entry; the host has made room for
// two entries per row of the list in front of the launch, and an entry past cap is counted and not stored all the same.
// The trip count of the loop is uniform per workgroup, so the two barriers of an append are met by all four waves.
__global__ __launch_bounds__(256) void mirror_pack_kernel(const smafa_hit *__restrict__ list, unsigned long long total_rows,
                                                          uint32_t p0, uint32_t S, uint32_t R,
                                                          const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ pos_of, uint32_t shift,
                                                          unsigned long long *__restrict__ entries,
                                                          uint32_t *__restrict__ rows, unsigned long long cap,
                                                          unsigned long long *total) {
    __shared__ uint32_t s_wave[2][4];
    __shared__ unsigned long long s_first[2];
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    uint32_t set = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total_rows; base += stride, set ^= 1u) {
        const unsigned long long i = base + threadIdx.x;
        smafa_hit h = {0, 0, 0};
        bool keep = false;
        if (i < total_rows) {
            h = list[i];
            keep = piece::keep_once(h, p0, S, R, order, pos_of);
        }
        const unsigned long long slot = piece::block_append(keep, total, 2u, s_wave, s_first, set);
        if (keep && slot + 1ull < cap) {
            const uint32_t a = h.query, b = h.subject;
            const unsigned long long dd = (unsigned long long)h.dist << 32;
            if (shift) {
                entries[slot] = ((unsigned long long)a << shift) | dd | b;
                entries[slot + 1] = ((unsigned long long)b << shift) | dd | a;
            } else {
                entries[slot] = dd | b;
                entries[slot + 1] = dd | a;
                rows[slot] = a;
                rows[slot + 1] = b;
            }
        }
    }
}

// the row of sorted entry i, in either form
__device__ __forceinline__ uint32_t row_of(const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ rows,
                                           uint32_t shift, unsigned long long i) {
    return rows ? rows[i] : (uint32_t)(sorted[i] >> shift);
}

// lower[i], i = 0 .. n: the number of sorted entries whose row is below i — where row i's entries begin, and for a row
// without entries where the next row's do (lower[n] = count).  One thread per row and a binary search of <= 31 steps: a
// store of 10M rows with 200 000 entries has millions of rows between two entries, and nobody fills such a gap in a loop.
__global__ __launch_bounds__(256) void row_bounds_kernel(const unsigned long long *__restrict__ sorted,
                                                         const uint32_t *__restrict__ rows, uint32_t shift,
                                                         unsigned long long count, uint32_t n,
                                                         unsigned long long *__restrict__ lower) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    unsigned long long lo = 0, hi = count;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if ((unsigned long long)row_of(sorted, rows, shift, mid) < i) lo = mid + 1;
        else hi = mid;
    }
    lower[i] = lo;
}

// cut[i] = min(the degree of row i, k) for i < n, and a zero behind them: the exclusive sum over n + 1 ends in the total
__global__ __launch_bounds__(256) void cut_degrees_kernel(const unsigned long long *__restrict__ lower, uint32_t n, uint32_t k,
                                                          unsigned long long *__restrict__ cut) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const unsigned long long deg = i < n ? lower[i + 1] - lower[i] : 0ull;
    cut[i] = deg < k ? deg : (unsigned long long)k;
}

// One thread per sorted entry.  Its rank within its row is its index minus lower[row]; the first k of a row leave for
// offsets[row] + rank (no cut: offsets is lower, and the entry keeps its index).  dists may be nullptr.
__global__ __launch_bounds__(256) void emit_kernel(const unsigned long long *__restrict__ sorted,
                                                   const uint32_t *__restrict__ rows, uint32_t shift, unsigned long long count,
                                                   const unsigned long long *__restrict__ lower,
                                                   const unsigned long long *__restrict__ offsets, uint32_t k,
                                                   unsigned long long cap, uint32_t *__restrict__ neighbours,
                                                   uint32_t *__restrict__ dists) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned long long e = sorted[i];
        const uint32_t row = row_of(sorted, rows, shift, i);
        const unsigned long long rank = i - lower[row];
        if (rank >= k) continue;
        const unsigned long long at = offsets[row] + rank;
        if (at >= cap) continue;  // (the host launches this only where the total fits)
        neighbours[at] = (uint32_t)e;
        if (dists) dists[at] = rows ? (uint32_t)(e >> 32) : (uint32_t)(e >> 32) & ((1u << (shift - 32u)) - 1u);
    }
}

}  // namespace smafa_nb

// piece.hip.h — what every kernel that reads a self-join piece list shares (join.hip.h and its consumers: components, levels,
// density, peaks, neighbours, delta, forest, reach, chimera): the row format, the two list forms, and the appends — and, for the
// kernels of those headers that read no piece list (the flatten, settle, jump and seed kernels), the one wave idiom they repeated,
// wave_first / wave_count.  Device helpers only, all force-inlined; no kernel lives here.
//
// The row format.  A RAW piece list (self_join.hip.h: join_pieces) holds rows {query = record number of the query row in its span,
// subject = subject NUMBER, dist}: every pair the scan of the piece found, self-pairs and — for subjects inside or (block index)
// in front of the block — mirror images and repeats included.  A span at positions p0 .. is dealt into S interleaved blocks of up
// to R rows (store_records_kernel writes record (i % S) * R + i / S for position p0 + i), so record q is position
// piece_pos() = p0 + (q % R) * S + q / R, and order[] takes a position to its subject number.  The delta join's pieces are the
// same rows with S = 1, R = 0xffffffff and order = its own row list.
// The two list forms.  The KEPT list (J.kept) holds rows {a, b, dist} in subject numbers, each unordered pair once: a kernel that
// reads either is given order == nullptr for the kept list (p0, S, R unused) and reads a row's first subject through pair_of().
// The exactly-once rule.  A pair of positions a < b is met as (a, b) by the block that holds a and, where b's block sees a at
// all, again as (b, a): keep_once() keeps a row iff position(query) < position(subject), which keeps each pair once and drops the
// self-pairs, whichever scan kernel produced the list and however the store was cut.
// The appends.  A kernel that moves rows to a list reserves room on one 8-byte total, which is exact at any capacity: every
// flagged row is counted, the CALLER stores only where its slot is below its capacity.  wave_append(): one atomicAdd per wave
// that has a flagged lane.  block_append(): one per workgroup of four waves and loop iteration, through LDS.  The ORDER in which
// rows land depends on arrival; the kernels' own comments say why nothing that reads them depends on it.
#pragma once

#include "kernels.hip.h"

namespace piece {

// the position of record `query` of a raw row in the sorted store
__device__ __forceinline__ uint32_t piece_pos(uint32_t query, uint32_t p0, uint32_t S, uint32_t R) {
    return p0 + (query % R) * S + query / R;
}

// the exactly-once rule on a raw row; a kept row's query becomes its subject number (another position than the subject's:
// another subject number)
__device__ __forceinline__ bool keep_once(smafa_hit &h, uint32_t p0, uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                          const uint32_t *__restrict__ pos_of) {
    const uint32_t qpos = piece_pos(h.query, p0, S, R);
    const bool keep = qpos < pos_of[h.subject];
    if (keep) h.query = order[qpos];
    return keep;
}

// the subject number of the row's query in either list form; the other one is h.subject
__device__ __forceinline__ uint32_t pair_of(const smafa_hit &h, uint32_t p0, uint32_t S, uint32_t R, const uint32_t *__restrict__ order) {
    return order ? order[piece_pos(h.query, p0, S, R)] : h.query;
}

// whether this lane is the first of its wave with `flag` set: the one lane that acts for all of them
__device__ __forceinline__ bool wave_first(bool flag) {
    const unsigned long long mask = __ballot(flag);
    return flag && smafa::lanes_below(mask) == 0u;
}

// *counter += the number of lanes of the wave with `flag` set: one atomicAdd, by the first of them
template <class T>
__device__ __forceinline__ void wave_count(bool flag, T *counter) {
    const unsigned long long mask = __ballot(flag);
    if (flag && smafa::lanes_below(mask) == 0u) atomicAdd(counter, (T)__builtin_popcountll(mask));
}

// The slot of a flagged lane behind one reservation per wave on *counter: ballot, one atomicAdd by lane 0 (none where no lane
// is flagged), the broadcast, and the lane's rank among the flagged ones.  Every lane of the wave must call it; what a lane
// without the flag gets back is no slot of its own.
__device__ __forceinline__ unsigned long long wave_append(bool flag, unsigned long long *counter) {
    const unsigned long long mask = __ballot(flag);
    unsigned long long first = 0;
    if (mask != 0ull) {
        if ((threadIdx.x & 63u) == 0u) first = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
        first = smafa::shfl_u64(first, 0);
    }
    return first + smafa::lanes_below(mask);
}

// The slot of a flagged lane behind ONE reservation per workgroup of four waves and call: every wave ballots, the four counts
// meet in s_wave[set], thread 0 adds per_row times their sum to *counter (nothing where it is zero), and a lane's slot is what
// that returned plus per_row times its rank in the workgroup.  Every thread must call it the same number of times (two barriers
// per call): the caller's loop has a trip count that is uniform per workgroup, and flips `set` between 0 and 1 every iteration.
// Why two sets: a wave that is already publishing its count of iteration k + 1 writes the set that the slower waves, still
// reading iteration k, do not look at, and nobody reaches iteration k + 2 before everybody has passed the first barrier of k + 1.
__device__ __forceinline__ unsigned long long block_append(bool flag, unsigned long long *counter, uint32_t per_row,
                                                           uint32_t (*s_wave)[4], unsigned long long *s_first, uint32_t set) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_wave[set][wave] = (uint32_t)__builtin_popcountll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = s_wave[set][0] + s_wave[set][1] + s_wave[set][2] + s_wave[set][3];
        s_first[set] = all ? atomicAdd(counter, (unsigned long long)per_row * all) : 0ull;
    }
    __syncthreads();
    uint32_t rank = smafa::lanes_below(mask);
    for (uint32_t w = 0; w < wave; w++) rank += s_wave[set][w];
    return s_first[set] + (unsigned long long)per_row * rank;
}

}  // namespace piece

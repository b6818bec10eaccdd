// consensus.hip.h — kernels of the CONSENSUS of every labelled cluster of a resident store (engine.hip: smafa_db_consensus_launch).
// The definition is include/smafa_amd.h's; in short: the distinct values of labels[] other than SMAFA_NONE are the groups, in
// ascending order; codes[k][c] is the code most members of group k hold at source column c, a tie to the smallest code; div[i]
// the number of columns where row i differs from its group's consensus; nearest[k] the member with the smallest (div, number).
//
// This is the one self-store call that reads the planes themselves rather than the join's pairs: planes[tile][p][w][slot], the
// packed column order perm[] and the per-column re-coding tab[] (kernels.hip.h: pack_rows_kernel), and order[] (position -> subject).
// Its kernels live in `consensus::`, not in a `smafa_xx::` namespace: the censuses of tests/ pin every namespace that begins
// with `smafa` to the kernels it holds today.
//
//   mark_groups_kernel     per row: mark[labels[i]] = 1; the smallest row whose label is neither SMAFA_NONE nor a subject number
//                          goes to *bad by atomicMin.  An exclusive sum over mark[0 .. n] gives dense[] and, at dense[n], K.
//   group_ids_kernel       per value r with mark[r]: ids[dense[r]] = r
//   group_keys_kernel      per POSITION p of the store: key = dense[labels[order[p]]], or K for an unlabelled row and for the
//                          positions of the last tile that hold no subject; value = p.  One stable radix sort over the bits of K
//                          puts the positions of a group side by side, ascending: neighbours in the sorted list are neighbours
//                          in the store's tiles.
//   segment_bounds_kernel  per sorted entry: where the key changes, seg_begin[key] = the entry's index; seg_begin[K] = the
//                          number of labelled rows, M.
//   tally_vote_kernel      the hot kernel.  One wave64 per WINDOW of `chunk` sorted entries.  Lanes are packed columns: 64 of them
//                          at a time (two plane words), all windows of columns one after another.  The wave walks the pieces
//                          of groups inside its window; per piece the counters lds[stored code][lane] start at zero, every
//                          member's plane words are loaded once (lane i loads member i of a batch of 64, readlane hands them
//                          round), and lane c raises the counter of the code it sees.  A group that lies inside the window is
//                          voted on the spot; a piece of a group that crosses a window's edge adds its counters to the table of
//                          the window in which the group begins — at most one group crosses each edge, so there are at most
//                          ceil(n / chunk) tables of 32 x 32W counters, never one per group.  Integer adds commute: the table
//                          does not depend on the order in which the pieces arrive.
//   vote_tables_kernel     one wave per window whose last entry belongs to a group that begins in it and goes on behind it:
//                          the same vote, from the table.
//   measure_kernel         per labelled sorted entry: the row's plane words against its group's consensus RECORD (the consensus in
//                          the store's own bit-plane form, P x W words, written by the vote): popcount(OR_p(S_p ^ C_p)), the
//                          scan's distance.  div[order[p]] gets it, and (div << 32 | subject) goes to the group's slot by
//                          atomicMin — one atomic per wave where the whole wave is one group's.
//   finish_groups_kernel   per group: sizes[k] from seg_begin[], nearest[k] from the slot's low word.
//
// The vote.  Lane c of column window h stands for packed column j = 64h + c, source column perm[j].  It walks the SOURCE codes v
// in ascending order and reads the counter of tab[perm[j]][v]: the first greatest count wins, which is the smallest source code
// among the most frequent — the tie rule of the definition, N (4) included.  Columns j >= L are padding: they write nothing and
// their record bits are zero, as the rows' are.
//
// Who writes what: codes[k][·], the record of k and the slot of k belong to group k; a group is voted by exactly one wave
// (tally_vote_kernel where it lies inside a window, else vote_tables_kernel); tables are only added to (atomicAdd) in
// tally_vote_kernel and only read in vote_tables_kernel, behind the kernel boundary.  No flags, no spinning, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smafa_amd.h"

namespace consensus {

constexpr uint32_t kTile = 256;         // positions per wave tile (scan_plan.h: kWaveTile)
constexpr uint32_t kCodes = 32;         // counters per column: a stored code has at most five bits
constexpr uint32_t kWavesPerBlock = 4;  // tally_vote_kernel: four waves, 8 KB of counters each

__global__ __launch_bounds__(256) void mark_groups_kernel(const uint32_t *__restrict__ group_of, uint32_t n, uint32_t *mark, uint32_t *bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = group_of[i];
    if (r == SMAFA_NONE) return;
    if (r < n) mark[r] = 1u;  // (every writer writes 1)
    else atomicMin(bad, i);
}

__global__ __launch_bounds__(256) void group_ids_kernel(const uint32_t *__restrict__ mark, const uint32_t *__restrict__ dense, uint32_t n,
                                                        uint32_t *__restrict__ ids) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && mark[r]) ids[dense[r]] = r;
}

// n_pos positions (whole tiles), n of them hold a subject
__global__ __launch_bounds__(256) void group_keys_kernel(const uint32_t *__restrict__ group_of, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ dense, uint32_t n, uint32_t n_pos, uint32_t K,
                                                         uint32_t *__restrict__ keys, uint32_t *__restrict__ positions) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pos) return;
    uint32_t key = K;
    if (p < n) {
        const uint32_t r = group_of[order[p]];
        if (r != SMAFA_NONE) key = dense[r];  // (r < n: the gate behind mark_groups_kernel)
    }
    keys[p] = key;
    positions[p] = p;
}

// seg_begin[0 .. K]: every group has a member, so every key below K occurs
__global__ __launch_bounds__(256) void segment_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t n_pos, uint32_t K,
                                                             uint32_t *__restrict__ seg_begin) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_pos) return;
    const uint32_t k = keys[s];
    if (s == 0u || keys[s - 1u] != k) seg_begin[k] = s;
    if (s + 1u == n_pos && k != K) seg_begin[K] = n_pos;  // no unlabelled position at all
}

// The vote of one group over one window of 64 packed columns.  count(stored code) is this lane's counter; rec: the group's record.
template <int P, class Count>
__device__ __forceinline__ void vote_window(Count count, uint32_t h, uint32_t lane, uint32_t L, uint32_t W, const uint32_t *__restrict__ perm,
                                            const uint8_t *__restrict__ tab, uint8_t *__restrict__ codes_k, uint32_t *__restrict__ rec) {
    constexpr uint32_t kSource = P == 5 ? 28u : P == 3 ? 5u : 4u;  // source codes a store of P planes can hold
    const uint32_t col = 64u * h + lane;
    const bool live = col < L;
    const uint32_t sc = live ? perm[col] : 0u;
    const uint8_t *tcol = tab + (size_t)sc * 32u;
    uint32_t best = 0u, best_count = 0u, best_stored = 0u;
    if (live) {
#pragma unroll
        for (uint32_t v = 0; v < kSource; v++) {
            const uint32_t stored = tcol[v];
            const uint32_t have = stored < (1u << P) ? count(stored) : 0u;
            if (have > best_count) best = v, best_count = have, best_stored = stored;
        }
        codes_k[sc] = (uint8_t)best;
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
        const unsigned long long bits = __ballot(live && ((best_stored >> p) & 1u));
        if (lane == 0u) {
            rec[(uint32_t)p * W + 2u * h] = (uint32_t)bits;
            if (2u * h + 1u < W) rec[(uint32_t)p * W + 2u * h + 1u] = (uint32_t)(bits >> 32);
        }
    }
}

// keys / positions: the sorted list; seg_begin[K] = M labelled entries.  Window t = entries [t * chunk, (t + 1) * chunk) below M.
// tables: one per window, [32][32 W] counters, zero on entry; recs: [K][P][W]; codes: [K][L]
template <int P>
__global__ __launch_bounds__(256) void tally_vote_kernel(const uint32_t *__restrict__ planes, const uint32_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ positions, const uint32_t *__restrict__ seg_begin,
                                                         uint32_t K, uint32_t chunk, uint32_t n_windows, uint32_t L, uint32_t W,
                                                         const uint32_t *__restrict__ perm, const uint8_t *__restrict__ tab,
                                                         uint32_t *tables, uint32_t *__restrict__ recs, uint8_t *__restrict__ codes) {
    __shared__ uint32_t lds[kWavesPerBlock][kCodes][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + wave));
    if (t >= n_windows) return;
    const uint32_t M = seg_begin[K];
    const uint64_t lo64 = (uint64_t)t * chunk;
    if (lo64 >= M) return;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + chunk < M ? lo64 + chunk : M);
    uint32_t(*cnt)[64] = lds[wave];
    constexpr uint32_t kStored = 1u << P;
    for (uint32_t h = 0; 2u * h < W; h++) {
        const bool two = 2u * h + 1u < W;  // the window's second word exists
        for (uint32_t s = lo; s < hi;) {
            const uint32_t g = keys[s];  // wave-uniform
            const uint32_t g_begin = seg_begin[g], g_end = seg_begin[g + 1u];
            const uint32_t end = g_end < hi ? g_end : hi;
            const bool whole = g_begin >= lo && g_end <= hi;
#pragma unroll
            for (uint32_t v = 0; v < kStored; v++) cnt[v][lane] = 0u;
            for (uint32_t base = s; base < end; base += 64u) {
                const uint32_t live = end - base < 64u ? end - base : 64u;
                uint32_t w0[P], w1[P];
#pragma unroll
                for (int p = 0; p < P; p++) w0[p] = w1[p] = 0u;
                if (lane < live) {  // lane i: member base + i
                    const uint32_t pos = positions[base + lane];
                    const uint32_t *row = planes + ((size_t)(pos / kTile) * P * W + 2u * h) * kTile + (pos & (kTile - 1u));
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        w0[p] = row[(size_t)p * W * kTile];
                        if (two) w1[p] = row[(size_t)p * W * kTile + kTile];
                    }
                }
                for (uint32_t i = 0; i < live; i++) {
                    uint32_t code = 0u;
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)w0[p], (int)i);
                        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)w1[p], (int)i);
                        code |= (((lane < 32u ? a : b) >> (lane & 31u)) & 1u) << p;
                    }
                    cnt[code][lane] += 1u;  // this lane's own counter: no atomics inside the wave
                }
            }
            if (whole) {
                vote_window<P>([&](uint32_t stored) { return cnt[stored][lane]; }, h, lane, L, W, perm, tab, codes + (size_t)g * L,
                               recs + (size_t)g * P * W);
            } else if (lane < 32u || two) {  // the group crosses an edge: to the table of the window it begins in
                uint32_t *table = tables + (size_t)(g_begin / chunk) * (kCodes * 32u * W) + 64u * h + lane;
#pragma unroll
                for (uint32_t v = 0; v < kStored; v++) {
                    const uint32_t have = cnt[v][lane];
                    if (have) atomicAdd(table + (size_t)v * 32u * W, have);
                }
            }
            s = end;
        }
    }
}

// one wave per window: the group of the window's last entry, where it begins in this window and goes on in the next
template <int P>
__global__ __launch_bounds__(64) void vote_tables_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ seg_begin, uint32_t K,
                                                         uint32_t chunk, uint32_t L, uint32_t W, const uint32_t *__restrict__ perm,
                                                         const uint8_t *__restrict__ tab, const uint32_t *__restrict__ tables,
                                                         uint32_t *__restrict__ recs, uint8_t *__restrict__ codes) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint32_t M = seg_begin[K];
    const uint64_t edge = ((uint64_t)t + 1u) * chunk;  // first entry of the next window
    if (edge >= M) return;
    const uint32_t g = keys[edge - 1u];
    if (keys[edge] != g || seg_begin[g] / chunk != t) return;
    const uint32_t *table = tables + (size_t)t * (kCodes * 32u * W);
    for (uint32_t h = 0; 2u * h < W; h++) {
        const bool mine = lane < 32u || 2u * h + 1u < W;  // (a column of a word the planes do not have: padding, never read)
        vote_window<P>([&](uint32_t stored) { return mine ? table[(size_t)stored * 32u * W + 64u * h + lane] : 0u; }, h, lane, L, W, perm, tab,
                       codes + (size_t)g * L, recs + (size_t)g * P * W);
    }
}

// slots: nullptr where no nearest member is asked for; div likewise
__global__ __launch_bounds__(256) void measure_kernel(const uint32_t *__restrict__ planes, const uint32_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ positions, const uint32_t *__restrict__ seg_begin, uint32_t K,
                                                      uint32_t P, uint32_t W, const uint32_t *__restrict__ recs,
                                                      const uint32_t *__restrict__ order, uint32_t *__restrict__ div,
                                                      unsigned long long *slots) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = s < seg_begin[K];
    uint32_t g = K;
    unsigned long long mine = ~0ull;
    if (live) {
        g = keys[s];
        const uint32_t pos = positions[s];
        const uint32_t *row = planes + (size_t)(pos / kTile) * P * W * kTile + (pos & (kTile - 1u));
        const uint32_t *rec = recs + (size_t)g * P * W;
        uint32_t d = 0u;
        for (uint32_t w = 0; w < W; w++) {
            uint32_t m = 0u;
            for (uint32_t p = 0; p < P; p++) m |= row[(size_t)(p * W + w) * kTile] ^ rec[p * W + w];
            d += (uint32_t)__builtin_popcount(m);
        }
        const uint32_t subject = order[pos];
        if (div) div[subject] = d;
        mine = ((unsigned long long)d << 32) | subject;
    }
    if (!slots) return;
    // a wave that is all one group's: its minimum, one atomic
    const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    if (__all(live && g == g0)) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(mine >> 32), off, 64);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)mine, off, 64);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            mine = other < mine ? other : mine;
        }
        if ((threadIdx.x & 63u) == 0u) atomicMin(slots + g0, mine);
    } else if (live) {
        atomicMin(slots + g, mine);
    }
}

__global__ __launch_bounds__(256) void finish_groups_kernel(const uint32_t *__restrict__ seg_begin, const unsigned long long *__restrict__ slots,
                                                            uint32_t K, uint32_t *__restrict__ sizes, uint32_t *__restrict__ nearest) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    sizes[k] = seg_begin[k + 1u] - seg_begin[k];
    if (nearest) nearest[k] = (uint32_t)slots[k];
}

}  // namespace consensus

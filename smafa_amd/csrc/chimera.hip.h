// chimera.hip.h — kernels of the CHIMERA CHECK of a resident store (engine.hip: smafa_db_self_chimeras_launch): which rows are a
// heavier row's head on another heavier row's tail (two-parent bimeras, as UNOISE, UCHIME de novo and isBimeraDenovo remove
// them behind a denoising partition).  The definition is include/smafa_amd.h's; in short, with D the bound, F the fold and
// weight[] counted as smafa_db_self_peaks counts it (or given by the caller):
//   p is an ELIGIBLE PARENT of q iff p != q, both weights are non-zero, dist(q, p) <= D, weight[p] > weight[q] and
//                          weight[p] >= F * weight[q] (in 64 bits);
//   pre(q, p), suf(q, p)   the lengths of the common prefix and suffix of the two rows in SOURCE column order;
//   left[q]                the eligible p of greatest (pre(q, p), -p), right[q] the same with suf;
//   flags[q] = 1           iff q has an eligible parent and pre(q, left[q]) + suf(q, right[q]) >= L.
// The self-join's driver finds the pairs (join.hip.h, the scan kernels unchanged) and smafa_pk::init_peaks_kernel (mode 0) and
// smafa_pk::weigh_keep_kernel weigh and keep them exactly as the peaks call does (peaks.hip.h); the kernels here are what
// follows, in a namespace of their own — not a `smafa_xx::` one: the censuses of tests/ pin every namespace that begins with
// `smafa` to the kernels it holds today:
//   init_sides_kernel    left[i] = right[i] = 0: "no parent yet"
//   offer_sides_kernel   phase 2, the hot kernel, per row {a, b, dist} of a list: plain loads of both weights decide whether the
//                        pair is eligible and which row is q; an ineligible pair leaves before any plane load.  For an eligible
//                        pair the P x W plane words of both rows are gathered through pos_of[] (planes[tile][p][w][slot], as
//                        consensus.hip.h reads them), per word m_w = OR_p(q_p ^ p_p) has one bit per differing PACKED column —
//                        at most dist bits in all — and each bit is walked with ctz and mapped to its source column through
//                        perm[], keeping the smallest and the greatest: pre = the smallest, suf = L - 1 - the greatest.  perm[]
//                        is copied to LDS once per workgroup where it fits (it does up to L = 12 288; beyond, it is read
//                        from memory).  q is then offered (pre << 32) | (SMAFA_NONE - p) on its left slot and
//                        (suf << 32) | (SMAFA_NONE - p) on its right.
//   verdict_kernel       phase 3, per row: the two slots unpacked, the flag, the parents, the lengths and the weight written
//                        (each optional array only when asked for), the flagged rows counted by ballot per wave, the four
//                        waves adding in LDS, then one atomicAdd per workgroup.
//
// Three phases with kernel boundaries between them.  A weight is known only once EVERY pair has been weighed (or the caller's
// weights have been copied in, behind the join), so no offer can run while a weigh is still running: phase 1 is the whole join,
// phase 2 reads the kept pair list in one launch where that list held every kept row, or is the join once more with
// offer_sides_kernel as the piece consumer (self_join.hip.h decides from the kept total).  Every load of weight[] here comes
// after the last write to it, and is plain.
//
// What is atomic, and why the answer does not depend on the order the rows arrive in.
//   left[], right[]  8 B each per subject, (length << 32) | (0xFFFFFFFF - parent): comparing two slots as integers compares
//             (length, -parent), the order of the definition.  atomicMax only: a slot only ever goes UP, from 0 to the maximum
//             of what was offered to it, in whatever order — and the offers of a row are exactly one per eligible parent,
//             each a pure function of the two rows' planes and numbers.  0 is never offered (the low word of an offer is
//             0xFFFFFFFF - p >= 1), so a slot is 0 iff the row has no eligible parent, and then so is its other slot.  A
//             relaxed agent-scope load comes first — a slot that is high enough already costs no atomic; an out-of-date value
//             can only be too low, and then the atomicMax decides.  atomicMax is idempotent, so offer_sides_kernel is as correct
//             on a raw piece list — self-pairs (skipped: a == b), mirror images and (block index) repeats included — as on the
//             kept list, where each pair appears once in one orientation: the second join needs no filter.
//   the count one atomicAdd per workgroup of verdict_kernel; integer addition commutes.
// No flags between workgroups, no spinning, no hand-off, no inline assembly: the only synchronisation is the atomics above and
// the kernel boundaries.
#pragma once

#include "piece.hip.h"

namespace chimera {

constexpr uint32_t kTile = 256;           // positions per wave tile (scan_plan.h: kWaveTile)
constexpr uint32_t kPermLdsWords = 12288;  // perm[] goes to LDS while 32 W is at most this (48 KB)

__global__ __launch_bounds__(256) void init_sides_kernel(unsigned long long *__restrict__ left, unsigned long long *__restrict__ right,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) left[i] = right[i] = 0ull;
}

// Over either list form (piece.hip.h: pair_of), as smafa_pk::climb_kernel.
// planes: the store's, P planes of W words per position; perm: 32 W entries, packed column -> source column; L: source columns;
// perm_words: 32 W where perm[] is to be copied to LDS (the launch then gives 4 x perm_words bytes of it), else 0.
__global__ __launch_bounds__(256) void offer_sides_kernel(const smafa_hit *__restrict__ list, unsigned long long total, uint32_t p0,
                                                          uint32_t S, uint32_t R, const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ pos_of, const uint32_t *__restrict__ weight,
                                                          uint32_t fold, const uint32_t *__restrict__ planes, uint32_t P, uint32_t W,
                                                          uint32_t L, const uint32_t *__restrict__ perm, uint32_t perm_words,
                                                          unsigned long long *left, unsigned long long *right) {
    extern __shared__ uint32_t s_perm[];
    for (uint32_t j = threadIdx.x; j < perm_words; j += blockDim.x) s_perm[j] = perm[j];
    __syncthreads();
    const uint32_t *const column = perm_words ? s_perm : perm;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const smafa_hit h = list[i];
        const uint32_t a = piece::pair_of(h, p0, S, R, order), b = h.subject;
        if (a == b) continue;
        const uint32_t wa = weight[a], wb = weight[b];
        if (wa == wb || wa == 0u || wb == 0u) continue;
        const uint32_t q = wa < wb ? a : b, p = wa < wb ? b : a;
        const unsigned long long wq = wa < wb ? wa : wb, wp = wa < wb ? wb : wa;
        if (wp < (unsigned long long)fold * wq) continue;
        const uint32_t qpos = pos_of[q], ppos = pos_of[p];
        const uint32_t *qrow = planes + (size_t)(qpos / kTile) * P * W * kTile + (qpos & (kTile - 1u));
        const uint32_t *prow = planes + (size_t)(ppos / kTile) * P * W * kTile + (ppos & (kTile - 1u));
        uint32_t first = L, last = 0u;  // the smallest and the greatest differing source column
        for (uint32_t w = 0; w < W; w++) {
            uint32_t m = 0u;
            for (uint32_t pl = 0; pl < P; pl++) m |= qrow[(size_t)(pl * W + w) * kTile] ^ prow[(size_t)(pl * W + w) * kTile];
            const uint32_t cols = L > 32u * w ? L - 32u * w : 0u;  // columns of this word that exist; the rest is padding
            if (cols < 32u) m &= (1u << cols) - 1u;
            while (m) {
                const uint32_t c = column[32u * w + (uint32_t)__builtin_ctz(m)];
                m &= m - 1u;
                first = c < first ? c : first;
                last = c > last ? c : last;
            }
        }
        if (first >= L) continue;  // no differing column: equal rows have equal weights, and never come this far
        const unsigned long long low = (unsigned long long)(SMAFA_NONE - p);
        const unsigned long long pre = ((unsigned long long)first << 32) | low, suf = ((unsigned long long)(L - 1u - last) << 32) | low;
        if (__hip_atomic_load(left + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pre) atomicMax(left + q, pre);
        if (__hip_atomic_load(right + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < suf) atomicMax(right + q, suf);
    }
}

// Behind the last offer, a launch of its own: left[], right[] and weight[] are final and read-only here.  Every output but
// flags may be nullptr.
__global__ __launch_bounds__(256) void verdict_kernel(const unsigned long long *__restrict__ left, const unsigned long long *__restrict__ right,
                                                      const uint32_t *__restrict__ weight, uint32_t n, uint32_t L,
                                                      uint32_t *__restrict__ flags, uint32_t *__restrict__ left_parent,
                                                      uint32_t *__restrict__ left_len, uint32_t *__restrict__ right_parent,
                                                      uint32_t *__restrict__ right_len, uint32_t *__restrict__ weights,
                                                      unsigned long long *n_chimeras) {
    __shared__ uint32_t s_flagged;
    if (threadIdx.x == 0u) s_flagged = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool flagged = false;
    if (i < n) {
        const unsigned long long l = left[i], r = right[i];
        const uint32_t pre = (uint32_t)(l >> 32), suf = (uint32_t)(r >> 32);
        flagged = l != 0ull && (unsigned long long)pre + suf >= L;
        flags[i] = flagged ? 1u : 0u;
        if (left_parent) left_parent[i] = l ? SMAFA_NONE - (uint32_t)l : SMAFA_NONE;
        if (left_len) left_len[i] = pre;
        if (right_parent) right_parent[i] = r ? SMAFA_NONE - (uint32_t)r : SMAFA_NONE;
        if (right_len) right_len[i] = suf;
        if (weights) weights[i] = weight[i];
    }
    const unsigned long long mask = __ballot(flagged);
    if (flagged && __builtin_popcountll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0)
        atomicAdd(&s_flagged, (uint32_t)__builtin_popcountll(mask));
    __syncthreads();
    if (threadIdx.x == 0u && s_flagged) atomicAdd(n_chimeras, (unsigned long long)s_flagged);
}

}  // namespace chimera

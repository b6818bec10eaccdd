// join.hip.h — kernels of the self-join of a resident store (engine.hip: smafa_db_self_launch): every unordered pair of
// the store's own subjects within a bound, exactly once.  The join runs the scan kernels of kernels.hip.h unchanged — a
// block of POSITIONS of the sorted store is the query set, the tiles from the first one of the block's span to the end are
// the subjects — and adds the three kernels here, in a namespace of their own:
//   store_records_kernel   query records of a block straight from the bit-planes (a record IS the row's tile words in
//                          another order: no decode, no code table, no trip to the host)
//   inverse_order_kernel   pos_of[subject] = position, the inverse of order[], once per state of the store
//   join_filter_kernel     the exactly-once rule: a row of the block's list is kept iff position(query row) <
//                          position(subject row), and leaves with subject numbers, the smaller first
#pragma once

#include "piece.hip.h"

namespace smafa_join {

using smafa::kWaveTile;

constexpr int kRecWindow = 32;  // record words a workgroup transposes per pass: 256 rows x (32 + 1) words = 33 KiB of LDS

// Records of the rows at positions [p0, p1) (p1 <= subjects stored) — one SPAN of the join, cut into S interleaved blocks
// of up to R rows: the row at position p0 + i belongs to block i % S and is its row i / S, so its record is number
// (i % S) * R + i / S (engine.hip self_join: a block is then a contiguous range of records whose rows are spread over
// the whole span; S = 1: consecutive positions).  One workgroup per wave tile.  pack_rows_kernel writes the same word to planes[((tile*PS + p)*W + w)*256 + i] and to
// record slot qslot(PQ, W, p, w): per (plane, word) a wave reads the tile's 256 words as ONE 16-byte load per lane (1 KiB
// contiguous), scatters them into an LDS image of the tile's records, and the workgroup then writes the records out whole —
// consecutive lanes, consecutive words.  Slots no stored plane maps to (the bound slot, the padding up to QS, the plane a
// 2-plane nucleotide store does not hold) leave as zeros, as qset_fill's memset leaves them.  Records wider than
// kRecWindow words (the wide and generic kernels' stores) go through the same LDS image window by window.
// LDS rows: a lane holds positions 4*lane .. 4*lane + 3; position r lives in row (r & 3) * 64 + (r >> 2), so the four
// writes of a load go to rows lane, 64 + lane, ... at an odd row stride: no two lanes of a write share a bank.
__global__ __launch_bounds__(256) void store_records_kernel(const uint4 *__restrict__ planes, uint32_t PS, uint32_t PQ,
                                                            uint32_t W, uint32_t QS, uint32_t p0, uint32_t p1,
                                                            uint32_t S, uint32_t R, uint32_t *__restrict__ qrec) {
    __shared__ uint32_t img[kWaveTile * (kRecWindow + 1)];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = p0 / kWaveTile + blockIdx.x;
    const uint32_t base = tile * kWaveTile;
    const uint4 *src = planes + (size_t)tile * PS * W * 64;
    for (uint32_t s0 = 0; s0 < QS; s0 += kRecWindow) {
        const uint32_t sc = min((uint32_t)kRecWindow, QS - s0), stride = sc | 1u;
        for (uint32_t k = threadIdx.x; k < kWaveTile * stride; k += 256u) img[k] = 0u;
        __syncthreads();
        for (uint32_t k = wave; k < PS * W; k += 4u) {  // (plane, word) k: wave-uniform
            const uint32_t slot = (uint32_t)smafa::qslot((int)PQ, (int)W, (int)(k / W), (int)(k % W));
            if (slot < s0 || slot >= s0 + sc) continue;
            const uint4 v = src[(size_t)k * 64 + lane];
            uint32_t *d = img + lane * stride + (slot - s0);
            d[0] = v.x;
            d[64 * stride] = v.y;
            d[128 * stride] = v.z;
            d[192 * stride] = v.w;
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kWaveTile * sc; k += 256u) {
            const uint32_t r = k / sc, s = k - r * sc;
            const uint32_t pos = base + r;
            if (pos >= p0 && pos < p1) {
                const uint32_t i = pos - p0, rec = (i % S) * R + i / S;
                qrec[(size_t)rec * QS + s0 + s] = img[((r & 3u) * 64u + (r >> 2)) * stride + s];
            }
        }
        __syncthreads();
    }
}

// order[] is a permutation of 0..n-1 (position -> subject number): every pos_of entry is written exactly once
__global__ void inverse_order_kernel(const uint32_t *__restrict__ order, uint32_t n, uint32_t *__restrict__ pos_of) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) pos_of[order[p]] = p;
}

// A raw piece list under the exactly-once rule (piece.hip.h: the row format, keep_once).  Kept rows leave as {min, max of the
// two subject numbers, dist} through piece::wave_append on *out_count (zeroed by the host once per join); rows past cap are
// counted and not stored.
__global__ __launch_bounds__(256) void join_filter_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                          uint32_t p0, uint32_t S, uint32_t R,
                                                          const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ pos_of, smafa_hit *out,
                                                          unsigned long long cap, unsigned long long *out_count) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < total; base += stride) {
        const unsigned long long i = base + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool keep = false;
        if (i < total) {
            h = list[i];
            keep = piece::keep_once(h, p0, S, R, order, pos_of);
            if (keep) {
                const uint32_t a = h.query, b = h.subject;
                h.query = min(a, b);
                h.subject = max(a, b);
            }
        }
        const unsigned long long slot = piece::wave_append(keep, out_count);
        if (keep && slot < cap) out[slot] = h;
    }
}

}  // namespace smafa_join

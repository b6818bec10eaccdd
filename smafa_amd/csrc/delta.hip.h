// delta.hip.h — kernels of the DELTA self-join of a resident store (engine.hip: smafa_db_self_since_launch,
// smafa_db_self_components_update_launch): the pairs that the rows appended since a mark — subject numbers first_row .. n-1,
// "the new rows" — form with every row of the store, and the components they leave behind.  The driver (self_join.hip.h:
// delta_pass) makes query records of the new rows, a span of them at a time, and scans every block of a span against ALL
// tiles with the scan kernels as they are; the three kernels here, in a namespace of their own:
//   gather_records_kernel  query records of scattered rows of the sorted store, through pos_of[] (store_records_kernel
//                          transposes whole consecutive tiles and cannot)
//   delta_filter_kernel    the exactly-once rule on subject NUMBERS: a row {record r, subject s, dist} is kept iff
//                          s < rows[r] — no pos_of[], no full pass
//   seed_parents_kernel    parent[] of the union-find from the labels of the store as it was before the append, checked
#pragma once

#include "piece.hip.h"

namespace smafa_dl {

using smafa::kWaveTile;

// Records of the subjects first .. first + m - 1 — a span of the new rows — as records 0 .. m - 1 of qrec, and their
// subject numbers to rows_out[0 .. m) (the consumers' order[]: subject of the list's query r).  Subject s sits at position
// p = pos_of[s], tile p / 256, lane slot p % 256, and word (plane, w) of its record is the tile's word
// planes[((tile*PS + plane)*W + w)*256 + p%256], which pack_rows_kernel wrote to the record's slot qslot(PQ, W, plane, w).
// The reads cannot coalesce: consecutive words of ONE row lie 1 KiB apart, the price of tile-major bit-planes, and
// consecutive rows lie wherever the sort put them.  Thread t of the grid owns stored word k = t % (PS*W) of record
// t / (PS*W) — (plane, w) = (k / W, k % W), as store_records_kernel walks them — reads it and writes it to the slot
// qslot() names: one read, one write and no search per thread, whatever the record's width.  qslot() rises with w within
// a plane and the planes' slot ranges follow each other, so consecutive lanes write consecutive words of one record but
// for a step at the bound slot and at a plane's edge, and a wave's writes fall into the few cache lines of the records
// it covers.  Slots no stored plane maps to (the bound slot, the padding up to QS, the plane a 2-plane nucleotide store
// does not hold) are never written: the host zero-fills qrec in front, as it does for store_records_kernel's spans.
__global__ __launch_bounds__(256) void gather_records_kernel(const uint32_t *__restrict__ planes,
                                                             const uint32_t *__restrict__ pos_of, uint32_t PS, uint32_t PQ,
                                                             uint32_t W, uint32_t QS, uint32_t first, uint32_t m,
                                                             uint32_t *__restrict__ qrec, uint32_t *__restrict__ rows_out) {
    const uint32_t stored = PS * W;
    const unsigned long long words = (unsigned long long)m * stored, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += stride) {
        const uint32_t r = (uint32_t)(t / stored), k = (uint32_t)(t - (unsigned long long)r * stored);
        const uint32_t s = first + r, p = pos_of[s];
        if (k == 0u) rows_out[r] = s;
        const uint32_t slot = (uint32_t)smafa::qslot((int)PQ, (int)W, (int)(k / W), (int)(k % W));
        qrec[(size_t)r * QS + slot] = planes[((size_t)(p / kWaveTile) * stored + k) * kWaveTile + (p % kWaveTile)];
    }
}

// A piece's list holds rows {query = record r of the span, subject = subject NUMBER s, dist}: every row of the store within
// the bound of new row a = rows[base + r], the row itself included.  Kept iff s < a, and it leaves as {s, a, dist}:
//   an old partner (s < first_row <= a) is met once, by a's scan, and kept;
//   a pair of two new rows is met twice, once by each one's scan, and kept where the partner has the smaller number;
//   the self-pair (s == a) is dropped.
// So every pair {i < j, j >= first_row} leaves exactly once, whatever the positions of its rows and whichever kernel
// produced the list.  Output space as in join_filter_kernel: piece::wave_append on *out_count (zeroed by the host once per
// call); rows past cap are counted and not stored.
__global__ __launch_bounds__(256) void delta_filter_kernel(const smafa_hit *__restrict__ list, unsigned long long total,
                                                           uint32_t base, const uint32_t *__restrict__ rows, smafa_hit *out,
                                                           unsigned long long cap, unsigned long long *out_count) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x; at < total; at += stride) {
        const unsigned long long i = at + threadIdx.x;  // uniform trip count per workgroup
        smafa_hit h = {0, 0, 0};
        bool keep = false;
        if (i < total) {
            h = list[i];
            const uint32_t a = rows[base + h.query];
            keep = h.subject < a;
            h.query = h.subject;
            h.subject = a;
        }
        const unsigned long long slot = piece::wave_append(keep, out_count);
        if (keep && slot < cap) out[slot] = h;
    }
}

// parent[i] = labels[i] for i < first_row — the flat forest smafa_db_self_components left for the store's first first_row
// rows: every old row points at the smallest number of its set, which points at itself — and parent[i] = i behind it.
// parent[x] <= x holds from the start, as the union-find of components.hip.h needs.  What can be checked per row is:
// labels[i] <= i, labels[i] < first_row (implied by the first; kept for a label array that is shorter than claimed) and
// labels[labels[i]] == labels[i].  A row that fails is counted in *bad (one atomicAdd per wave) and seeded as its own
// root, so that nothing behind the kernel can follow a pointer out of parent[]; the host reads *bad at its first wait and
// fails the call before anything is written for the caller.
__global__ __launch_bounds__(256) void seed_parents_kernel(const uint32_t *__restrict__ labels, uint32_t first_row, uint32_t n,
                                                           uint32_t *__restrict__ parent, unsigned long long *bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool wrong = false;
    if (i < n) {
        uint32_t to = i;
        if (i < first_row) {
            const uint32_t l = labels[i];
            wrong = l > i || l >= first_row || labels[l] != l;
            if (!wrong) to = l;
        }
        parent[i] = to;
    }
    piece::wave_count(wrong, bad);
}

}  // namespace smafa_dl

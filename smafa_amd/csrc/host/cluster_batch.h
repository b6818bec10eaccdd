// cluster_batch.h — the three rules of the batched clustering (host/cluster.cpp) that every rank must evaluate alike: pure
// functions of exchanged quantities, without a device and without I/O, so a CPU test feeds them directly
// (tests/test_cluster_batch_model.py).
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/smafa_amd.h"  // smafa_hit

namespace smafa {
#pragma GCC visibility push(hidden)  // internal to the library: none of this is exported

// The sequential pass over one batch of nb records, in input order (src/cluster.rs:62-74 for every record of the batch).
//   old_d[nb], old_c[nb]  each record's nearest centroid among those known BEFORE the batch, lowest ordinal on ties, and its
//                         distance; UINT32_MAX in both: none within max_divergence (a listed one IS within it)
//   cand_pos[]            candidate ordinal -> batch position, ascending: exactly the positions without an old centroid
//   cand_hits[n_hits]     every (record, candidate) pair within max_divergence, ordered by (query, dist, subject); query is the
//                         batch position, subject the candidate ordinal
//   next_centroid         the ordinal the next new centroid gets
// -> centroid[nb], the centroid ordinal of every batch position, and became[], the batch positions that became centroids, in
//    order: became[k] is centroid next_centroid + k.
// A record chooses between its old centroid and the candidates EARLIER in the batch that did become centroids.  Those are
// numbered in batch order and the rows of a record are ordered (dist, candidate), so its first admissible row is its best new
// centroid; every old centroid has a lower ordinal than any new one, so the new one must be strictly nearer to win — the
// reference's first minimum.  A record with nothing within max_divergence becomes a centroid itself.
inline void resolve_batch(size_t nb, const uint32_t *old_d, const uint32_t *old_c, const std::vector<uint32_t> &cand_pos,
                          const smafa_hit *cand_hits, size_t n_hits, uint32_t max_divergence, uint32_t next_centroid,
                          std::vector<uint32_t> &centroid, std::vector<uint32_t> &became) {
    std::vector<uint32_t> cand_centroid(cand_pos.size(), UINT32_MAX);  // candidate ordinal -> centroid ordinal it became (or none)
    centroid.assign(nb, UINT32_MAX);
    became.clear();
    size_t h = 0, next_cand = 0;
    for (size_t b = 0; b < nb; b++) {
        uint32_t best_d = old_d[b], best_c = old_c[b];
        while (h < n_hits && cand_hits[h].query < b) h++;
        for (size_t t = h; t < n_hits && cand_hits[t].query == b; t++) {
            const uint32_t c = cand_hits[t].subject;
            if (cand_pos[c] >= b || cand_centroid[c] == UINT32_MAX) continue;  // later record / not a centroid
            if (cand_hits[t].dist < best_d) {  // strict: an old centroid wins ties (lower index)
                best_d = cand_hits[t].dist;
                best_c = cand_centroid[c];
            }
            break;
        }
        if (best_c != UINT32_MAX && best_d <= max_divergence) {  // src/cluster.rs:62-68
            centroid[b] = best_c;
        } else {  // src/cluster.rs:69-74
            while (cand_pos[next_cand] != b) next_cand++;
            const uint32_t at = (uint32_t)b;
            cand_centroid[next_cand] = centroid[b] = next_centroid + (uint32_t)became.size();
            became.push_back(at);
        }
    }
}

// Where rank's slice of a batch of nb records starts; it ends where the next rank's starts.  Slices are contiguous and in rank
// order.
inline size_t slice_start(size_t nb, uint32_t rank, uint32_t world) { return nb * rank / world; }

// The size of the next batch after one of nb records with n_cand candidates and n_rows candidate rows.  The batch size follows
// the row volume: it grows, up to batch_cap, while the scans stay cheap, and shrinks, down to 256, on dense input.  (Exchanged
// quantities only, so every rank takes the same decision.)
inline size_t next_batch_size(size_t B, size_t batch_cap, size_t nb, size_t n_cand, size_t n_rows) {
    const size_t volume = (nb - n_cand) + n_rows;
    if (volume < (4u << 20) && B < batch_cap) return B * 2;
    if (volume > (16u << 20) && B > 256) return B / 2;
    return B;
}

#pragma GCC visibility pop
}  // namespace smafa

// subset.hip.h — kernels of the two calls that take rows OUT of a resident store: a subset of it as a new store
// (smafa_db_subset_launch) and its sequences back as code bytes (smafa_db_rows_launch).  Host side: subset_abi.hip.h.
//   keep_flags_kernel      per subject and per position: 1 where the row is kept (keep[] non-zero, or zero under `invert`)
//   move_rows_kernel       every kept row's P x W plane words to its new position, order[] renumbered, old_of_new[] written
//   run_ends_kernel        the kept rows in front of each boundary between the source's runs
//   unpack_rows_kernel<P>  m x L code bytes of listed (or consecutive) subjects: the inverse of smafa::pack_rows_kernel
// Why a subset needs no sort: positions are sorted by filter key within every run, and deleting rows from a sorted sequence
// leaves it sorted.  Two exclusive sums (hipCUB, over plain uint32) give every kept subject its new number and every kept
// position its new position; the zone words of the new tiles are recomputed by smafa::zone_kernel as it is.
// Included once by engine.hip, outside namespace smafa.
#pragma once

namespace subset {

constexpr uint32_t kTile = 256;  // subjects per wave tile (smafa::kWaveTile)
constexpr uint32_t kUnpackWaves = 4;           // waves per workgroup of unpack_rows_kernel
constexpr uint32_t kUnpackLdsPerWave = 8192;   // bytes of staged rows per wave: 64 rows of up to 128 columns at once
constexpr uint32_t kUnpackMaxColumns = 16384;  // one row must fit a wave's share of 64 KiB

// flag_subject[s] = subject s is kept, flag_position[p] = the subject at position p is; both hold n + 1 entries, the last one
// zero, so that the exclusive sums over them end in the kept total.
__global__ void keep_flags_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ order, uint32_t n, uint32_t invert,
                                  uint32_t *__restrict__ flag_subject, uint32_t *__restrict__ flag_position) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t fs = 0, fp = 0;
    if (i < n) {
        fs = ((keep[i] != 0u) ? 1u : 0u) ^ invert;
        fp = ((keep[order[i]] != 0u) ? 1u : 0u) ^ invert;  // (order[] is a permutation of 0 .. n-1)
    }
    flag_subject[i] = fs;
    flag_position[i] = fp;
}

// Thread i moves the row at OLD position i, if it is kept, to position new_position[i]: consecutive kept lanes write
// consecutive words of the new tile, the reads are the old tile's rows with holes.  planes[tile][P][W][256] on both sides;
// the new block was zero-filled, so the padding of its last tile stays zero.  new_number[] / new_position[] are the
// exclusive sums of keep_flags_kernel's flags (n + 1 entries each): entry i + 1 minus entry i is the flag.
// Thread i also writes old_of_new[] for SUBJECT i (old_of_new may be nullptr).
__global__ void move_rows_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t *__restrict__ order_in,
                                 uint32_t *__restrict__ order_out, const uint32_t *__restrict__ new_number,
                                 const uint32_t *__restrict__ new_position, uint32_t n, uint32_t PW, uint32_t *__restrict__ old_of_new) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (old_of_new) {
        const uint32_t s = new_number[i];
        if (new_number[i + 1] != s) old_of_new[s] = i;
    }
    const uint32_t p = new_position[i];
    if (new_position[i + 1] == p) return;  // dropped
    order_out[p] = new_number[order_in[i]];
    const uint32_t *s = in + (size_t)(i / kTile) * ((size_t)PW * kTile) + (i % kTile);
    uint32_t *d = out + (size_t)(p / kTile) * ((size_t)PW * kTile) + (p % kTile);
    for (uint32_t j = 0; j < PW; j++) d[(size_t)j * kTile] = s[(size_t)j * kTile];
}

// out[j] = new_position[ends[j]]: the kept rows in front of old position ends[j] (ends[j] <= n)
__global__ void run_ends_kernel(const uint32_t *__restrict__ new_position, const uint32_t *__restrict__ ends, uint32_t r,
                                uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < r) out[j] = new_position[ends[j]];
}

// The inverse of smafa::pack_rows_kernel.  A wave owns 64 output rows j0 .. j0 + 63 (row j: subject subjects[j], or first + j
// where subjects is nullptr).  Lane i finds row i's position through pos_of[] and, per 64-column slice h, loads that row's two
// words of every plane; then for each row i the wave reads them by readlane — wave-uniform 64-bit slices of the planes — and
// lane c takes bit c of each: the stored code of packed column 64h + c, which inv[source column][stored code] and perm[] turn
// into the source code at its source column.  The bytes are staged in LDS, R whole rows at a time, and leave the wave as one
// contiguous run of R x L bytes: dword stores where the destination is 4-aligned, bytes at the two ends.
// A listed subject >= n gives a row of 0xff and reads nothing of the store.  `lds_rows` = R (1 .. 64), the rows a wave's share
// of the dynamic LDS holds.
template <int P>
__global__ __launch_bounds__(kUnpackWaves * 64) void unpack_rows_kernel(const uint32_t *__restrict__ planes, const uint32_t *__restrict__ pos_of,
                                                                        const uint32_t *__restrict__ subjects, uint64_t first, uint64_t m,
                                                                        uint32_t n, uint32_t L, uint32_t W,
                                                                        const uint32_t *__restrict__ perm, const uint8_t *__restrict__ inv,
                                                                        uint32_t lds_rows, uint8_t *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t staged_rows[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t j0 = ((uint64_t)blockIdx.x * kUnpackWaves + wave) * 64u;
    if (j0 >= m) return;  // (no workgroup barrier below: a wave works alone)
    const uint32_t rows = (uint32_t)(m - j0 < 64u ? m - j0 : 64u);
    uint8_t *const mine = staged_rows + (size_t)wave * (((size_t)lds_rows * L + 15u) & ~(size_t)15u);
    bool listed = lane < rows, stored = false;
    uint32_t pos = 0;
    if (listed) {
        const uint64_t s = subjects ? (uint64_t)subjects[j0 + lane] : first + j0 + lane;
        stored = s < n;
        if (stored) pos = pos_of[s];  // < n
    }
    const unsigned long long absent = __ballot(listed && !stored);
    const uint32_t *const my_words = planes + (size_t)(pos / kTile) * ((size_t)P * W * kTile) + (pos % kTile);
    for (uint32_t g0 = 0; g0 < rows; g0 += lds_rows) {
        const uint32_t g1 = g0 + lds_rows < rows ? g0 + lds_rows : rows;
        const bool in_group = stored && lane >= g0 && lane < g1;
        for (uint32_t h = 0; h * 2u < W; h++) {
            uint32_t lo[P], hi[P];
#pragma unroll
            for (int p = 0; p < P; p++) {
                lo[p] = hi[p] = 0u;
                if (in_group) {
                    lo[p] = my_words[((size_t)p * W + 2u * h) * kTile];
                    if (2u * h + 1u < W) hi[p] = my_words[((size_t)p * W + 2u * h + 1u) * kTile];
                }
            }
            const uint32_t col = 64u * h + lane;
            const bool has_col = col < L;
            const uint32_t scol = has_col ? perm[col] : 0u;  // < L
            const uint8_t *const icol = inv + (size_t)scol * 32u;
            for (uint32_t i = g0; i < g1; i++) {  // wave-uniform
                uint32_t code = 0;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)lo[p], (int)i);
                    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)hi[p], (int)i);
                    const unsigned long long slice = ((unsigned long long)b << 32) | a;
                    code |= (uint32_t)((slice >> lane) & 1ull) << p;
                }
                if (has_col) mine[(size_t)(i - g0) * L + scol] = ((absent >> i) & 1ull) ? (uint8_t)0xff : icol[code];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the staged bytes are read by other lanes of this wave
        __builtin_amdgcn_wave_barrier();
        // the group's bytes, contiguous in `codes`
        uint8_t *const dst = codes + (j0 + g0) * L;
        const uint32_t total = (g1 - g0) * L;
        uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
        if (head > total) head = total;
        const uint32_t n_words = (total - head) / 4u, tail_at = head + n_words * 4u;
        if (lane < head) dst[lane] = mine[lane];
        for (uint32_t d = lane; d < n_words; d += 64u) {
            const uint8_t *const b = mine + head + 4u * d;
            *reinterpret_cast<uint32_t *>(dst + head + 4u * d) =
                (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        if (lane < total - tail_at) dst[tail_at + lane] = mine[tail_at + lane];
        __builtin_amdgcn_wave_barrier();  // (the next group overwrites them)
    }
}

}  // namespace subset

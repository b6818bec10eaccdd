// The body of one chunk pass of scan_zone_kernel (kernels.hip.h), included there once per place it runs from: everything it names
// is the kernel's.  PLAIN and FULL are compile-time constants of the including scope, qc is the chunk's first query.
        const uint32_t nqc = FULL ? (uint32_t)kChunk : min((uint32_t)kChunk, qb1 - qc);
        const bool more = FULL || qc + kChunk < qb1;
        const uint2 head_cur = head_next;
        if (more) {  // in flight while this chunk is computed
            if (DIRECT) {
                head_next = load_head(qc + kChunk);
            } else {
                dma(buf ^ 1, qc + kChunk);  // every wave passed the barrier that ended the last use of that buffer
                if (!FIXED) nu_next = load_bound(qc + kChunk);
            }
        }
        if (PLAIN || active) {
            // (kSplit keeps no chunk counter: the chunk's number in its block follows from qc)
            const uint32_t cn = kSplit ? (qc - qb0) / (uint32_t)kChunk : chunk_no;
            const bool probe = PLAIN || (a.use_filter && (filter_on || (cn & 15u) == 0));
            if (probe) {
                uint32_t passes = 0;  // (query, tile) pairs of this chunk that needed the exact comparison
                // ---- zone level: lane i holds [f0 f1 ~bound ..] of query i of the chunk
                uint4 head = make_uint4(0u, 0u, 0u, 0u);  // lanes past the chunk: ~bound = 0 never passes
                if (DIRECT) head.x = head_cur.x, head.y = head_cur.y;
                else if (lane < nqc) head = stage[buf][lane * RV];
                const uint32_t hq0 = head.x, hq1 = W > 1 ? head.y : 0u;
                const uint32_t hnu = lane < nqc ? (FIXED ? nu0 : nu_lds[buf][lane]) : 0u;
                // (opaque copy: the comparisons against it are redone per chunk — one s_cmp each — instead of being hoisted
                // out of the chunk loop as T lane masks that then live in spilled VGPR lanes)
                uint32_t nl = PLAIN ? (uint32_t)T : n_live;
                if constexpr (!PLAIN) asm volatile("" : "+s"(nl));
                // Tile by tile, unrolled (the rare levels' address math stays inside their branch thanks to the opaque
                // tile number below; a run-time tile loop cost 4 % on aa and 27 % on nt at bound 3 in per-tile
                // bookkeeping — profiles/r02_zone_variants.txt).
                // (Round 3: the body is a function of the compile-time tile slot, called under `if (nl > t)` — as a loop with a
                // `break` and a `continue` the compiler threaded a state variable through the four bodies: ~10 scalar
                // instructions of pure control flow between two tiles, which counts where few queries survive a tile —
                // nucleotides at bound 3: scalar instructions 1.5 per 1024 pairs against 1.7 vector ones.)
                auto zone_keys = [&](auto slot) -> unsigned long long {
                    constexpr uint32_t t = decltype(slot)::value;
                    const uint32_t zc = zc0[t], zm = zm0[t];
                    const uint32_t d0 = (hq0 ^ zc) & (kMaskInVgpr ? zmv[t] : zm);  // the columns counted
                    uint32_t u = __builtin_popcount(d0) + hnu;
                    uint32_t d1 = 0;
                    if (zone_w1) {
                        const uint32_t zc1 = NS > 0 ? zc1s[t] : (uint32_t)__builtin_amdgcn_readlane((int)vz.z, (int)t);
                        const uint32_t zm1 = NS > 0 ? zm1s[t] : (uint32_t)__builtin_amdgcn_readlane((int)vz.w, (int)t);
                        d1 = (hq1 ^ zc1) & zm1;
                        u += __builtin_popcount(d1);
                    }
                    unsigned long long m = __ballot((int32_t)u < 0);  // queries of the chunk this tile cannot exclude
                    if constexpr (NS > 0) {
                        // ---- key test (where enough queries survive for it to pay): ~u = the survivor's budget b
                        if ((uint32_t)__builtin_popcountll(m) >= a.key_gate) {
                            bool pass = false;
                            if ((int32_t)u < 0) {
                                const uint32_t s0 = hq0 ^ d0, s1 = hq1 ^ d1;  // the query, the tile's shared bits substituted
                                const uint32_t ky = key_y(s0), kx = key_x(s1);
                                const uint32_t vy = km[(t * NS + 0) * KW + (ky >> 5)];
                                const uint32_t vx = km[(t * NS + 1) * KW + (kx >> 5)];
                                uint32_t found = ((vy >> (ky & 31u)) & 1u) + ((vx >> (kx & 31u)) & 1u);
                                const uint32_t kz = key_z(s1);  // (set Z behind the other two: the compiler's schedule follows the text)
                                const uint32_t vz_ = km[(t * NS + 2) * KW + (kz >> 5)];
                                found += (vz_ >> (kz & 31u)) & 1u;
                                pass = found + ~u >= (uint32_t)NS;
                            }
                            m = __ballot(pass);
                        }
                    }
                    return m;
                };
                auto survivors = [&](auto slot, unsigned long long m) {
                    constexpr uint32_t t = decltype(slot)::value;
                    const uint32_t tile = tile0 + t;
                    const uint4 ft = f0[t];
                    if constexpr (kSplit) {
                        // (a ballot is uniform, but behind the wave's choice of body the compiler no longer proves it for the scalar
                        // operand below; on a scalar register this is no instruction)
                        m = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m) |
                            (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32;
                    }
                    while (m != 0ull) {
                        const int i = __builtin_ctzll(m);
                        asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(i));  // m &= ~(1 << i) in ONE scalar op (m & (m - 1): three)
                        // ---- level 1: word 0 of the filter plane.  The query's word and ~bound come out of lane i as
                        // scalar operands.  Measured alternatives (profiles/r02_zone_variants.txt): two survivors per
                        // iteration 13 % slower; the word via an LDS broadcast read (all-VGPR xors) 4 % slower, 16 %
                        // slower when software-pipelined; the word copied to a VGPR first (v_mov, all-VGPR xors): no change.
                        const uint32_t q0w = (uint32_t)__builtin_amdgcn_readlane((int)hq0, i);
                        const uint32_t nu = FIXED ? nu0 : (uint32_t)__builtin_amdgcn_readlane((int)hnu, i);
                        const uint32_t u0 = __builtin_popcount(ft.x ^ q0w) + nu;
                        const uint32_t u1 = __builtin_popcount(ft.y ^ q0w) + nu;
                        const uint32_t u2 = __builtin_popcount(ft.z ^ q0w) + nu;
                        const uint32_t u3 = __builtin_popcount(ft.w ^ q0w) + nu;
                        if (__ballot((int32_t)(or3(u0, u1, u2) | u3) < 0) == 0ull) continue;
                        // the rare levels get the tile number through an opaque copy: otherwise the compiler hoists
                        // their ~25 address computations out of this loop into the per-tile path every chunk pays
                        // for (6 % of the launch)
                        uint32_t tile_r = tile;
                        asm volatile("" : "+s"(tile_r));
                        // ... and the chunk parity likewise: the LDS addresses of the staged record and of the row stage
                        // (five scalar instructions) were being formed in front of EVERY tile's survivor loop (nt 3.52 ->
                        // 3.35 ms — profiles/r04_zone_variants.txt)
                        int buf_r = __builtin_amdgcn_readfirstlane(buf);
                        asm volatile("" : "+s"(buf_r));
                        uint32_t qw[RS];
                        if constexpr (kL2Lanes) {
                            // ---- level 2, two filter words, no memory but the wave's own: the query's word 1 out of lane i like
                            // word 0, the tile's word 1 from its home; the record is read behind it, for level 3
                            const uint32_t q1w = (uint32_t)__builtin_amdgcn_readlane((int)hq1, i);
                            uint4 v;
                            if constexpr (kF1Home == 1) v = f1_home[t * 64 + lane];
                            else v = planes[(size_t)tile_r * (PS * W * 64) + (FP * W + 1) * 64 + lane];
                            const uint32_t each = fold_sign<2>(ft.x ^ q0w, ft.y ^ q0w, ft.z ^ q0w, ft.w ^ q0w, [&](int) { return v; },
                                                               [&](int) { return q1w; }, nu);
                            if (__ballot((int32_t)each < 0) == 0ull) continue;
                            read_record(reinterpret_cast<const uint4 *>(qrec + (size_t)(qc + (uint32_t)i) * RS), qw);
                            qw[BS] = nu;
                            passes++;
                            stream_compare(tile_r, qw, qc + (uint32_t)i, buf_r);
                            continue;
                        }
                        // ---- level 2 (rare): the filter plane folded over all its words, words 1.. from L2/HBM
                        if (DIRECT) read_record(reinterpret_cast<const uint4 *>(qrec + (size_t)(qc + (uint32_t)i) * RS), qw);
                        else read_record(&stage[buf_r][(uint32_t)i * RV], qw);
                        qw[BS] = nu;  // the staged record carries no bound
                        if (W > 1) {
                            const uint4 *src = planes + (size_t)tile_r * (PS * W * 64) + (FP * W) * 64 + lane;
                            const uint32_t each = fold_sign<W>(ft.x ^ qw[0], ft.y ^ qw[0], ft.z ^ qw[0], ft.w ^ qw[0], [&](int w) { return src[w * 64]; },
                                                               [&](int w) { return qw[qslot(PQ, W, FP, w)]; }, nu);
                            if (__ballot((int32_t)each < 0) == 0ull) continue;
                        }
                        // ---- level 3: all planes, exactly
                        passes++;
                        stream_compare(tile_r, qw, qc + (uint32_t)i, buf_r);
                    }
                };
                static_assert(T <= 8, "tile slots are spelled out below");
                auto each_slot = [&](auto &&f) {  // f(tile slot as a compile-time constant), slots 0 .. T - 1 in order
                    f(std::integral_constant<uint32_t, 0>{});
                    if constexpr (T > 1) f(std::integral_constant<uint32_t, 1>{});
                    if constexpr (T > 2) f(std::integral_constant<uint32_t, 2>{});
                    if constexpr (T > 3) f(std::integral_constant<uint32_t, 3>{});
                    if constexpr (T > 4) f(std::integral_constant<uint32_t, 4>{});
                    if constexpr (T > 5) f(std::integral_constant<uint32_t, 5>{});
                    if constexpr (T > 6) f(std::integral_constant<uint32_t, 6>{});
                    if constexpr (T > 7) f(std::integral_constant<uint32_t, 7>{});
                };
                if constexpr (kHoist) {
                    // Two phases: zone level and key test of every tile slot first (one survivor mask per slot, in scalars),
                    // then the survivor loops — what the first phase keeps per chunk is dead before the first loop.
                    unsigned long long ms[T];
                    if (PLAIN || key_hoist) {
                        // the keys (v_bfe_u32 takes the low 5 bits of one as the bit position by itself) and their bitmap words' LDS
                        // addresses from the head alone; per tile there remain 3 gathers at immediate offsets.  (The address is
                        // formed in one opaque instruction: as plain arithmetic the compiler re-adds the base in front of every
                        // gather.)
                        // (Computed for every chunk, 9 VALU, also where no tile reaches the gate or the test is off, gate 65.)
                        const uint32_t ky = key_y(hq0), kx = key_x(hq1), kz = key_z(hq1);
                        typedef const __attribute__((address_space(3))) uint32_t *lds_u32;
                        const uint32_t km_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)km;
                        auto word_of = [&](uint32_t key) -> uint32_t {  // LDS address of word key >> 5 of (tile slot 0, set 0)
                            uint32_t at;
                            asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(at) : "v"(key >> 5), "s"(km_lds));
                            return at;
                        };
                        const uint32_t ay = word_of(ky), ax = word_of(kx), az = word_of(kz);
                        // lanes past the block are masked out of the ballot (scalar) instead of out of ~bound (per lane)
                        // (a FULL chunk has no such lane)
                        const unsigned long long in_block = FULL ? ~0ull : ~0ull >> (64u - nqc);
                        auto hoisted = [&](auto with_w1) {
                            // zone level of every slot; slots past the range keep an empty mask (an active wave's slot 0 is
                            // inside it) and, in the last wave alone, gather from their own bitmaps for nothing
                            uint32_t u[T];
                            bool test = false;
                            unsigned long long any = 0ull;
                            each_slot([&](auto slot) {
                                constexpr uint32_t t = decltype(slot)::value;
                                u[t] = __builtin_popcount((hq0 ^ zc0[t]) & (kMaskInVgpr ? zmv[t] : zm0[t])) + nu0;
                                if (decltype(with_w1)::value) u[t] += __builtin_popcount((hq1 ^ zc1s[t]) & zm1s[t]);
                                unsigned long long m = __builtin_amdgcn_ballot_w64((int32_t)u[t] < 0);
                                if constexpr (!FULL) m &= in_block;
                                ms[t] = PLAIN || t == 0u || nl > t ? m : 0ull;
                                if constexpr (PLAIN) any |= m;
                                else test = test || (uint32_t)__builtin_popcountll(ms[t]) >= a.key_gate;
                            });
                            // PLAIN: one count for the chunk — the queries that survive ANY slot against the gate (0: always,
                            // 65: never, like the count per slot; in between the test runs for a superset of the chunks, and
                            // it only ever removes pairs that have no hit)
                            if constexpr (PLAIN) test = (uint32_t)__builtin_popcountll(any) >= a.key_gate;
                            if (test) {
                                // all gathers under their slots' survivors, nothing between them that waits: ONE LDS latency per
                                // chunk.  (Slot by slot behind a gate branch each, every tile waited out its own latency — the
                                // form of profiles/r06_zone_hoist.txt; see profiles/r10_zone_level2.txt.)  General body: lanes
                                // that did not survive keep 0 = nothing found, so their u stays >= 0 below.
                                // PLAIN: no zero fill — what a lane that did not survive holds is unspecified; it counts at most NS
                                // found sets on u >= 0, which stays above -NS, and ms[t] already leaves the lane out.
                                uint32_t g[T][3];
                                each_slot([&](auto slot) {
                                    constexpr uint32_t t = decltype(slot)::value;
                                    if constexpr (PLAIN) asm volatile("" : "=v"(g[t][0]), "=v"(g[t][1]), "=v"(g[t][2]));
                                    else g[t][0] = g[t][1] = g[t][2] = 0u;
                                    if ((int32_t)u[t] < 0) {
                                        g[t][0] = *(lds_u32)(uintptr_t)(ay + ((t * NS + 0) * KW) * 4u);
                                        g[t][1] = *(lds_u32)(uintptr_t)(ax + ((t * NS + 1) * KW) * 4u);
                                        g[t][2] = *(lds_u32)(uintptr_t)(az + ((t * NS + 2) * KW) * 4u);
                                    }
                                });
                                // found sets + budget ~u >= NS  <=>  u - found < -NS
                                each_slot([&](auto slot) {
                                    constexpr uint32_t t = decltype(slot)::value;
                                    const uint32_t found = __builtin_amdgcn_ubfe(g[t][0], ky, 1) + __builtin_amdgcn_ubfe(g[t][1], kx, 1) +
                                                           __builtin_amdgcn_ubfe(g[t][2], kz, 1);
                                    ms[t] &= __builtin_amdgcn_ballot_w64((int32_t)(u[t] - found) < -(int32_t)NS);
                                });
                            }
                        };
                        // word 1's share of the zone level under a scalar branch: it is rare (zone_w1)
                        if (!PLAIN && zone_w1) hoisted(std::true_type{});
                        else hoisted(std::false_type{});
                    } else {
                        each_slot([&](auto slot) {
                            constexpr uint32_t t = decltype(slot)::value;
                            ms[t] = t == 0u || nl > t ? zone_keys(slot) : 0ull;
                        });
                    }
                    each_slot([&](auto slot) { survivors(slot, ms[decltype(slot)::value]); });
                } else {
                    each_slot([&](auto slot) {
                        constexpr uint32_t t = decltype(slot)::value;
                        if (nl > t) survivors(slot, zone_keys(slot));
                    });
                }
                // an exact comparison from L2 costs ~60 VALU per (query, tile) pair, the dense walk below ~25 for EVERY
                // pair of the chunk (4 tiles x nqc): switch when more than ~2/5 of the pairs got that far
                // (PLAIN: the filter is on and the rule can only turn it off; its three scalar instructions run in every pass — the
                // compiler keeps them there whether or not a test of passes != 0 stands in front)
                if constexpr (kSplit) {
                    // (the count is the same in every lane; said so, or the choice of body that hangs on it counts as divergent and
                    // everything behind it is compiled for lanes that disagree)
                    const uint32_t n_exact = (uint32_t)__builtin_amdgcn_readfirstlane((int)passes);
                    if constexpr (PLAIN) {
                        if (n_exact * 5u > nqc * 8u) filter_on = false;
                    } else {
                        filter_on = n_exact * 5u <= nqc * 8u;
                    }
                } else {
                    filter_on = passes * 5u <= nqc * 8u;
                }
            } else {
                // dense neighbourhoods: one pass over the chunk per tile, that tile's planes in registers
                for (uint32_t t = 0; t < (uint32_t)T; t++) {
                    const uint32_t tile = tile0 + t;
                    if (t >= n_live) break;
                    uint4 s[PS * W];
                    uint32_t tile_d = tile;  // opaque: the walk's addresses are formed here, not kept (spilled) from the prologue
                    asm volatile("" : "+s"(tile_d));
                    const uint4 *src = planes + (size_t)tile_d * (PS * W * 64) + lane;
#pragma unroll
                    for (int i = 0; i < PS * W; i++) s[i] = src[i * 64];
                    const uint4 *rec = DIRECT ? reinterpret_cast<const uint4 *>(qrec + (size_t)qc * RS) : &stage[buf][0];
                    for (uint32_t i = 0; i < nqc; i++, rec += RV) {
                        uint32_t qw[RS];
                        read_record(rec, qw);
                        const uint32_t U = FIXED ? a.thr0 : ~nu_lds[buf][i];
                        uint32_t d[4];
#pragma unroll
                        for (int w = 0; w < W; w++) {
                            uint32_t extra = 0;
#pragma unroll
                            for (int p = PS; p < PQ; p++) extra |= qw[qslot(PQ, W, p, w)];
                            uint32_t m0 = extra, m1 = extra, m2 = extra, m3 = extra;
#pragma unroll
                            for (int p = 0; p < PS; p++) {
                                const uint4 v = s[p * W + w];
                                const uint32_t qv = qw[qslot(PQ, W, p, w)];
                                m0 = or_xor(m0, v.x, qv);
                                m1 = or_xor(m1, v.y, qv);
                                m2 = or_xor(m2, v.z, qv);
                                m3 = or_xor(m3, v.w, qv);
                            }
                            d[0] = (w ? d[0] : 0u) + __builtin_popcount(m0);
                            d[1] = (w ? d[1] : 0u) + __builtin_popcount(m1);
                            d[2] = (w ? d[2] : 0u) + __builtin_popcount(m2);
                            d[3] = (w ? d[3] : 0u) + __builtin_popcount(m3);
                        }
                        const uint32_t subj0 = tile * kWaveTile + lane * 4u;
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (d[k] <= U && subj0 + k < a.n_subjects) {
                                if (DIRECT) emit_direct(a, qc + i, subj0 + k, d[k]);
                                else emit(a, rs, buf, qc + i, subj0 + k, d[k]);
                            }
                    }
                }
                load_filter();  // not kept across the walk (its registers hold the tile meanwhile): fetched again
            }
        }
        if (!DIRECT) {
            if (more && !FIXED && tid < (uint32_t)kChunk) nu_lds[buf ^ 1][tid] = nu_next;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the next chunk's DMA has landed
            __syncthreads();
            if (a.hits) flush_rows(a, rs, buf);
        }

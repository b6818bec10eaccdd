"""The automatic query block of a chunked zone launch is whole chunks (engine.h: query_block_size; engine.hip: launch_tiles).

scan_zone_kernel walks a query block in chunks of 64 queries, and a block that ends mid-chunk pays for a whole one: the metric's
6 blocks of 1 667 queries each ended in a chunk of 3.  The automatic size is now rounded up to a multiple of 64 for launches that
take the zone kernel with more than 64 queries; smafa_set_query_block stays exact.  On the CPU: the sizes, from the header
compiled for the host.  On the GPU: a batch of 2 060 queries against test_gpu_zone_level2.py's small store (79 tiles, one of
52 rows, 600 identical rows) is split 8 ways, 258 queries each, which rounds up to 320 and so to 7 blocks — 6 x 320 + 140, the last
one still ending mid-chunk at the batch's end — where the exact override of 258 gives 8: the block count `last_scan_plan` reports
pins the engine's rounding, and both give the oracle's rows byte for byte.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
import smafa_amd
from test_gpu_zone_level2 import N_SMALL, Letters, make_store, pack_on_host, planted_classes, read_packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 64  # kernels.hip.h: kChunk
NQ = 2060  # 8 blocks of 258 -> 320: 7 blocks


def test_automatic_query_block_is_whole_chunks(tmp_path):
    """the metric's shape (10M rows at 2 tiles per wave, 10 000 queries, 256 CUs), small shapes, and overrides, which come back unchanged"""
    src = tmp_path / "qb.cpp"
    src.write_text(
        '#include <cstdio>\n#include "%s"\n'
        "int main() {\n"
        "    const unsigned cases[][5] = {{0, 256, 4883, 10000, 64}, {0, 256, 4883, 10000, 1}, {0, 256, 10, 202, 64}, {0, 256, 10, 65, 64},\n"
        "                                 {0, 304, 20000, 125000, 64}, {0, 256, 10, 2060, 64}, {96, 256, 10, 202, 64}, {1667, 256, 4883, 10000, 64},\n"
        "                                 {500, 256, 10, 202, 64}};\n"
        '    for (const auto &c : cases) printf("%%u\\n", smafa::query_block_size(c[0], c[1], c[2], c[3], c[4]));\n'
        "}\n" % os.path.join(ROOT, "smafa_amd", "csrc", "engine.h"))
    exe = str(tmp_path / "qb")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-o", exe, str(src)], check=True, capture_output=True, text=True)
    out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    metric, exact, small, tiny, big, two, o96, o1667, o_over = out
    assert exact == 1667 and metric == 1728  # 6 blocks of 1667 queries -> 5 x 1728 + 1360: 157 chunk passes instead of 162
    passes = lambda nq, qb: sum((min(qb, nq - b) + CHUNK - 1) // CHUNK for b in range(0, nq, qb))
    assert passes(10000, exact) == 162 and passes(10000, metric) == 157
    for qb in (metric, small, tiny, big, two):
        assert qb % CHUNK == 0 and qb > 0, out
    assert small == 256 and tiny == 128  # one block: the batch itself, rounded up (the kernel clips the block at the last query)
    assert two == 320 and -(-2060 // 320) == 7 and -(-2060 // 258) == 8  # 8 blocks of 258 -> 6 x 320 + 140
    assert (o96, o1667) == (96, 1667)  # smafa_set_query_block stays exact
    assert o_over == 202  # (an override above the batch is the batch, as before)


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet,L,bound", [(smafa_amd.ALPHABET_AA, 60, 5), (smafa_amd.ALPHABET_NT, 60, 3)])
def test_rounded_blocks_give_the_oracles_rows(tmp_path, alphabet, L, bound):
    smafa_amd.build()
    oracle.build()
    rng = np.random.default_rng(1200 * alphabet + L)
    ab = Letters(tmp_path, alphabet, L, rng)
    s = make_store(rng, ab, N_SMALL, L)
    packed = str(tmp_path / "s.packed")
    pack_on_host(str(tmp_path / "s.fa"), packed, s, alphabet)
    _, _, order, zone = read_packed(packed, L)
    q = []
    for tile in (0, 1, len(zone) - 1):  # test_gpu_zone_level2.py's classes next to the first tiles and the last
        q += planted_classes(rng, ab, s, order[tile * 256 : min((tile + 1) * 256, N_SMALL)], L)[0]
    while len(q) < NQ - 20:  # a few substitutions from a stored row
        r = s[rng.integers(0, N_SMALL)].copy()
        for c in rng.choice(L, size=int(rng.integers(0, bound + 2)), replace=False):
            r[c] = ab.random_sub(rng, r[c])
        q.append(r)
    q += list(ab.lc[rng.integers(0, len(ab.lc), size=(20, L))])  # far rows
    q = np.array(q, dtype=np.uint8)[rng.permutation(NQ)]  # rows in every chunk of both blocks
    want = oracle.scan_codes(s, q, bound)
    assert len(q) == NQ and len(np.unique(want["query"] // CHUNK)) == (NQ + CHUNK - 1) // CHUNK
    for override, n_blocks in ((0, 7), (258, 8)):
        store = smafa_amd.SubjectStore.load(packed)
        try:
            store.set_zone_level(2)
            store.set_query_block(override)
            got = store.scan(q, max_divergence=bound)
            kernel, plan = store.last_scan_kernel(), store.last_scan_plan()
        finally:
            store.close()
        assert kernel.startswith("smafa::scan_zone_kernel") and kernel.endswith("2, true, true>"), kernel
        assert plan["query_blocks"] == n_blocks, (override, plan)  # 7 only if the engine rounded 258 up to 320
        assert got.tobytes() == want.tobytes(), override

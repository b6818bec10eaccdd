"""The planted block-edge inputs of tests/index_edges.py, checked without a GPU: for every planted pair the distance — a
literal (a != b).sum() over the code bytes — and the mismatches per block, recomputed from the code bytes and perm, must be
what the pair's class says (tests/index_edges.py); and the oracle's rows for the planted queries hold every only_clean,
shared, rotating and straddle pair once, at its distance, and no none_clean or over pair.  This is what validates the rows
tests/test_gpu_index_edges.py expects before a GPU is involved."""
import zlib

import numpy as np
import pytest

import oracle
from index_edges import SHAPES, SIZES, IndexPlanter, block_columns, observed, small_store


def planter(kind, L, D, n):
    return IndexPlanter(kind, L, n, D, seed=zlib.crc32(repr((kind, L, D, n)).encode()))


def test_blocks_are_the_engines():
    """col_begin[b] = b * L / blocks: disjoint, in order, covering every packed column"""
    for _, L, D in SHAPES:
        blocks = block_columns(L, D + 1)
        assert blocks[0][0] == 0 and blocks[-1][1] == L
        assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and all(c1 > c0 for c0, c1 in blocks)
    assert block_columns(60, 6)[3] == (30, 40)  # columns 31 and 32: two words
    assert [c1 - c0 for c0, c1 in block_columns(120, 32)].count(3) == 8 and max(c1 - c0 for c0, c1 in block_columns(120, 32)) == 4
    assert all(c1 - c0 == 1 for c0, c1 in block_columns(20, 20))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,L,D", SHAPES, ids=["%s-%d-%d" % s for s in SHAPES])
def test_planted_pairs_are_what_their_class_says(kind, L, D, n):
    p = planter(kind, L, D, n)
    B, blocks = D + 1, p.blocks
    assert sorted(p.perm) == list(range(L))
    s, q = p.subjects(), p.queries()
    assert len(s) == n and len(q) >= 65 and q.max() < p.ql and s.max() < p.sl
    if kind == "nt3":
        assert p.first.max() < 4 and (p.second == 4).any()  # the first N arrives with the second append
    if kind == "nt2":
        assert (q == 4).any()  # N on the query side only
    assert p.host_rows[0] == n - 1  # the store's last row, alone in its tile where n = 1025
    seen = {}
    for pair in p.planted:
        dist, per_block = observed(p, pair)
        cls, args = pair["cls"], pair["args"]
        clean = {b for b in range(B) if per_block[b] == 0}
        assert dist == sum(per_block) == len(pair["cols"])
        differ = sorted(j for j in range(L) if s[pair["subject"]][p.perm[j]] != q[pair["query"]][p.perm[j]])
        assert differ == pair["cols"]
        seen.setdefault(cls, []).append(args)
        if cls == "only_clean":
            c, v = args
            assert dist == D and clean == {c} and all(per_block[b] == 1 for b in range(B) if b != c)
            assert differ == [blocks[b][v] - v for b in range(B) if b != c]  # first column (v = 0) / last column (v = 1)
        elif cls == "none_clean":
            assert dist == D + 1 and not clean and per_block == [1] * B
        elif cls == "over":
            assert dist == D + 1 and clean == {args[0]} and sorted(per_block) == [0] + [1] * (B - 2) + [2]
        elif cls == "shared":
            assert dist == args[0] and sum(1 for m in per_block if m) == (1 if args[0] else 0)
            assert len(clean) >= min(2, B - 1)
        elif cls == "rotating":
            Dp, start = args
            assert dist == Dp and all(per_block[b] == (1 if (b - start) % B < Dp else 0) for b in range(B))
        elif cls == "straddle":
            assert dist == 1 and differ == [args[0]]
            c0, c1 = blocks[[b for b in range(B) if per_block[b]][0]]
            assert any(c0 < e < c1 for e in (32, 64, 96)) and args[0] % 32 in (31, 0)
        else:
            raise AssertionError(cls)
    # every class the shape can hold is there, for every block / distance / start
    width = [c1 - c0 for c0, c1 in blocks]
    assert sorted(seen["only_clean"]) == [(c, v) for c in range(B) for v in (0, 1)]
    assert seen["none_clean"] == [()]
    assert sorted(seen.get("over", [])) == [(c,) for c in range(B) if any(width[b] >= 2 for b in range(B) if b != c)]
    assert sorted(seen.get("shared", [])) == [(d,) for d in range(D) if max(width) >= d]
    assert sorted(seen.get("rotating", [])) == [(Dp, st) for Dp in range(D) for st in range(B)]
    edges = [e for e in (32, 64, 96) if any(c0 < e < c1 for c0, c1 in blocks)]
    assert sorted(seen.get("straddle", [])) == sorted((j,) for e in edges for j in (e - 1, e))
    assert sorted(p.straddling_blocks()) == sorted({b for b, (c0, c1) in enumerate(blocks) for e in edges if c0 < e < c1})
    # the oracle's rows at the index's bound: each pair within it once, at its distance; the pairs past it absent
    want = oracle.scan_codes(s, q, D)
    rows = {}
    for r in want:
        key = (int(r["query"]), int(r["subject"]))
        assert key not in rows
        rows[key] = int(r["dist"])
    for pair in p.planted:
        key = (pair["query"], pair["subject"])
        if pair["cls"] in ("none_clean", "over"):
            assert key not in rows, pair
        else:
            assert rows.get(key) == len(pair["cols"]), pair
    # a lower bound's rows are the rows of bound D with dist <= that bound, in the same order (what the GPU test compares with)
    for Dp in sorted({0, D // 2, max(D - 1, 0)}):
        assert want[want["dist"] <= Dp].tobytes() == oracle.scan_codes(s, q, Dp).tobytes()


def test_shapes_hold_the_geometry_the_index_tests_are_for():
    """a block on two words at every word edge, 32 blocks of 3 to 4 columns, one column per block — among the shapes"""
    edges = set()
    for _, L, D in SHAPES:
        edges |= {e for e in (32, 64, 96) for c0, c1 in block_columns(L, D + 1) if c0 < e < c1}
    assert edges == {32, 64, 96}
    assert ("aa", 120, 31) in SHAPES and ("nt3", 120, 31) in SHAPES and ("aa", 20, 19) in SHAPES


@pytest.mark.parametrize("kind", ["nt2", "nt3", "aa"])
def test_small_store_inputs(kind):
    for n in (1, 200, 257):
        s, q = small_store(kind, 60, n, 5, seed=n)
        assert s.shape == (n, 60) and len(q) > 64
        assert kind == "aa" or (s == 4).any() == (kind == "nt3")
        assert len(oracle.scan_codes(s, q, 5)) > 0

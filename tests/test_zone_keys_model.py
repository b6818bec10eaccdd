"""CPU model of the pigeonhole key test of scan_zone_kernel<.., DIRECT> (kernels.hip.h, zone_key_sets).

A tile is a set of subjects; a subject and a query are rows of letter codes, and the filter plane is bit 0 of each code.  The
model forms what the kernel forms — the zone words {common bits, shared bits} of the tile, the count k of shared columns in
which the query differs, the budget b = bound - k, one bitmap of subject keys per key set, the query keys with the tile's
shared bits substituted — and applies the rule "found sets + b >= number of sets".  Checked against brute force: the key
test never rejects a tile that holds a hit, and zone level + key test + exact comparison give exactly the brute-force hits.
"""
from __future__ import annotations

import numpy as np
import pytest

BOUND = 5


def key_layout(L, kb):
    """(xmask, zlo) as launch_tiles sets them for an L-column two-word store"""
    n1 = min(L - 32, 32)
    xw = kb if n1 >= 2 * kb else n1 // 2
    return (1 << xw) - 1, xw


def filter_words(codes):
    """(word 0, word 1) of the filter plane of each row: bit j % 32 of word j // 32 = bit 0 of column j's code"""
    bits = (codes & 1).astype(np.uint64)
    w = np.zeros((codes.shape[0], 2), dtype=np.uint64)
    for j in range(codes.shape[1]):
        w[:, j // 32] |= bits[:, j] << np.uint64(j % 32)
    return w.astype(np.uint32)


def keys(w0, w1, L, kb, sets):
    xmask, zlo = key_layout(L, kb)
    ky = int(w0) >> (32 - kb)
    kx = int(w1) & xmask
    kz = (int(w1) >> zlo) & ((1 << kb) - 1)
    return (ky, kx, kz)[:sets]


def tile_passes(tile, q, bound, L, kb, sets, substitute=True):
    """zone level, then the key test: False = the tile cannot hold a hit of q"""
    fw = filter_words(tile)
    qw = filter_words(q[None, :])[0]
    k = 0
    d = []
    for w in range(2):
        col = fw[:, w]
        shared = int(np.bitwise_and.reduce(~col) | np.bitwise_and.reduce(col)) & 0xFFFFFFFF  # bits every subject agrees on
        common = int(col[0]) & shared
        dw = (int(qw[w]) ^ common) & shared
        k += bin(dw).count("1")
        d.append(dw)
    if k > bound:
        return False
    b = bound - k
    maps = [set() for _ in range(sets)]
    for r in fw:
        for s, key in enumerate(keys(r[0], r[1], L, kb, sets)):
            maps[s].add(key)
    s0 = int(qw[0]) ^ d[0] if substitute else int(qw[0])
    s1 = int(qw[1]) ^ d[1] if substitute else int(qw[1])
    found = sum(key in maps[s] for s, key in enumerate(keys(s0, s1, L, kb, sets)))
    return found + b >= sets


def dist(tile, q):
    return (tile != q[None, :]).sum(axis=1)


@pytest.mark.parametrize("L", [33, 44, 56, 60, 64])
@pytest.mark.parametrize("kb,sets", [(12, 3), (12, 2), (13, 3)])
def test_random_tiles_never_drop_a_hit(L, kb, sets):
    rng = np.random.default_rng(L * 100 + kb * 10 + sets)
    letters = 20
    checked = hits = rejected = 0
    for trial in range(300):
        n = int(rng.integers(4, 40))
        base = rng.integers(0, letters, size=L, dtype=np.uint8)
        tile = np.repeat(base[None, :], n, axis=0)
        free = rng.choice(L, size=int(rng.integers(2, L // 2)), replace=False)  # the columns the tile does not share
        tile[:, free] = rng.integers(0, letters, size=(n, len(free)), dtype=np.uint8)
        q = tile[int(rng.integers(0, n))].copy()
        for c in rng.choice(L, size=int(rng.integers(0, 2 * BOUND)), replace=False):
            q[c] = flip(q[c]) if rng.random() < 0.7 else rng.integers(0, letters)
        has_hit = bool((dist(tile, q) <= BOUND).any())
        passes = tile_passes(tile, q, BOUND, L, kb, sets)
        assert passes or not has_hit, (L, trial)
        checked += 1
        hits += has_hit
        rejected += not passes
    assert hits > 20 and rejected > 20, (checked, hits, rejected)  # both sides of the rule were exercised


def planted_tile(rng, L, n, shared_cols):
    """n subjects identical on shared_cols, random elsewhere; filter bits on shared_cols agree by construction"""
    letters = 20
    base = rng.integers(0, letters, size=L, dtype=np.uint8)
    tile = rng.integers(0, letters, size=(n, L), dtype=np.uint8)
    tile[:, shared_cols] = base[shared_cols]
    return tile


def flip(code):
    """another letter whose filter bit differs"""
    return (int(code) + 1) % 20


@pytest.mark.parametrize("L", [44, 56, 60, 64])
@pytest.mark.parametrize("kb,sets", [(12, 3), (12, 2), (13, 3)])
def test_adversarial_shared_column_mismatches(L, kb, sets):
    """D mismatches all in shared columns (each flips the filter bit, so k = D and b = 0), one or two of them inside a key set:
    the hit must survive — only the substitution of the tile's shared bits keeps it; D + 1 such mismatches are rejected."""
    rng = np.random.default_rng(L + kb + sets)
    xmask, zlo = key_layout(L, kb)
    xw = bin(xmask).count("1")
    key_cols = {
        "Y": list(range(32 - kb, 32)),
        "X": [32 + j for j in range(xw)],
        "Z": [32 + j for j in range(zlo, min(zlo + kb, L - 32))],
    }
    names = ["Y", "X", "Z"][:sets]
    dropped_without_substitution = 0
    for trial in range(120):
        inside = [names[trial % sets]] if trial % 2 else [names[trial % sets], names[(trial + 1) % sets]]
        chosen = []
        for nm in inside:
            chosen.append(int(rng.choice(key_cols[nm])))
        others = [c for c in range(L) if c not in chosen and all(c not in key_cols[nm] for nm in names)]
        chosen += [int(c) for c in rng.choice(others, size=BOUND + 1 - len(chosen), replace=False)]
        shared = sorted(set(chosen) | set(int(c) for c in rng.choice(L, size=L // 3, replace=False)))
        tile = planted_tile(rng, L, 24, shared)
        for extra in (0, 1):  # exactly at the bound, then one past it
            q = tile[3].copy()
            for c in chosen[: BOUND + extra]:
                q[c] = flip(q[c])
            d = dist(tile, q)
            want = bool((d <= BOUND).any())
            assert want == (extra == 0)
            assert tile_passes(tile, q, BOUND, L, kb, sets) == want, (L, trial, extra)
            if want and not tile_passes(tile, q, BOUND, L, kb, sets, substitute=False):
                dropped_without_substitution += 1
    # the placements are the ones a missing substitution gets wrong
    assert dropped_without_substitution > 60


@pytest.mark.parametrize("L", [33, 60])
def test_pipeline_equals_brute_force(L):
    """zone level + key test + exact comparison of the tiles that pass = every pair within the bound, no more"""
    rng = np.random.default_rng(7 + L)
    for trial in range(40):
        tile = planted_tile(rng, L, 32, sorted(rng.choice(L, size=L // 2, replace=False)))
        for _ in range(8):
            q = tile[int(rng.integers(0, 32))].copy()
            for c in rng.choice(L, size=int(rng.integers(0, BOUND + 3)), replace=False):
                q[c] = rng.integers(0, 20)
            d = dist(tile, q)
            want = np.nonzero(d <= BOUND)[0]
            got = np.nonzero(d <= BOUND)[0] if tile_passes(tile, q, BOUND, L, 12, 3) else np.zeros(0, dtype=np.int64)
            assert np.array_equal(got, want)

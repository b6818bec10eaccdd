"""CPU model of the hoisted key test of scan_zone_kernel<.., DIRECT> (kernels.hip.h: kHoist, key_hoist).

The kernel forms one flag per wave — no tile slot's zone masks (zm0, zm1) touch a key column — and, where it holds, takes a
query's three keys from its own filter words instead of from the words with the tile's shared bits substituted.  Checked here,
over random and adversarial zone words: the hoisted keys equal the substituted keys for every tile of the wave exactly when the
flag holds (for some query when it does not), the word address / bit position split the kernel uses addresses the same bitmap
bit, and the rewritten pass rule `u - found < -sets` is the rule `found + ~u >= sets`.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_zone_keys_model import key_layout, keys

M32 = 0xFFFFFFFF


def key_masks(L, kb, sets):
    """(word 0 bits, word 1 bits) that belong to a key set"""
    xmask, zlo = key_layout(L, kb)
    y = (M32 << (32 - kb)) & M32
    x = xmask
    z = (((1 << kb) - 1) << zlo) & M32 if sets > 2 else 0
    return y, x | z


def flag(zones, L, kb, sets):
    """the wave-uniform flag: OR over the tile slots of the keys of the zone masks is zero"""
    acc = 0
    for _, zm0, _, zm1 in zones:
        for k in keys(zm0, zm1, L, kb, sets):
            acc |= k
    return acc == 0


def substituted(q0, q1, zone):
    zc0, zm0, zc1, zm1 = zone
    return q0 ^ ((q0 ^ zc0) & zm0), q1 ^ ((q1 ^ zc1) & zm1)


def random_zone(rng, L, mode):
    """zone words {c0, m0, c1, m1} (c within m, bits past the row length clear); mode picks where the shared bits sit"""
    cols1 = (1 << (L - 32)) - 1 if L < 64 else M32
    if mode == "leading":  # a sorted store's tile: bits 0..k of word 0
        m0, m1 = (1 << int(rng.integers(0, 20))) - 1, 0
    elif mode == "sparse":
        m0 = int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32))
        m1 = int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32)) & cols1
    elif mode == "one_bit":  # a single shared column anywhere
        b = int(rng.integers(0, L))
        m0, m1 = (1 << b if b < 32 else 0), (1 << (b - 32) if b >= 32 else 0)
    else:  # "all": identical rows
        m0, m1 = M32, cols1
    c0 = int(rng.integers(0, 1 << 32)) & m0
    c1 = int(rng.integers(0, 1 << 32)) & m1
    return c0, m0, c1, m1


@pytest.mark.parametrize("L", [33, 37, 44, 56, 60, 64])
@pytest.mark.parametrize("kb,sets", [(12, 3), (12, 2), (13, 3)])
def test_hoisted_keys_equal_substituted_keys_exactly_when_the_flag_holds(L, kb, sets):
    rng = np.random.default_rng(L * 1000 + kb * 10 + sets)
    cols1 = (1 << (L - 32)) - 1 if L < 64 else M32
    held = broken = 0
    for trial in range(600):
        n_tiles = int(rng.integers(1, 5))
        mode = ("leading", "sparse", "one_bit", "all")[trial % 4]
        zones = [random_zone(rng, L, mode if t == trial % n_tiles else "leading") for t in range(n_tiles)]
        f = flag(zones, L, kb, sets)
        y, xz = key_masks(L, kb, sets)
        assert f == all((zm0 & y) == 0 and (zm1 & xz) == 0 for _, zm0, _, zm1 in zones)
        if f:
            held += 1
            for _ in range(20):
                q0, q1 = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) & cols1
                for z in zones:
                    assert keys(*substituted(q0, q1, z), L, kb, sets) == keys(q0, q1, L, kb, sets)
        else:
            broken += 1
            # some tile shares a key column: the query that differs from the tile there gets another key
            z = next(z for z in zones if (z[1] & y) or (z[3] & xz))
            q0, q1 = (z[0] ^ z[1]) & M32, (z[2] ^ z[3]) & cols1  # the complement of the common bits on every shared column
            assert keys(*substituted(q0, q1, z), L, kb, sets) != keys(q0, q1, L, kb, sets)
    assert held > 100 and broken > 100, (held, broken)


@pytest.mark.parametrize("L", [33, 37, 41, 44, 60, 64])
@pytest.mark.parametrize("kb", [12, 13])
def test_word_and_bit_of_a_key(L, kb):
    """address = key >> 5 (v_lshl_add_u32 on it), bit = the key's low 5 bits as v_bfe_u32 reads them from the whole key"""
    rng = np.random.default_rng(L + kb)
    cols1 = (1 << (L - 32)) - 1 if L < 64 else M32
    for _ in range(2000):
        q0, q1 = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) & cols1
        for key in keys(q0, q1, L, kb, 3):
            assert 0 <= key < (1 << kb)
            word, bit = key >> 5, key & 31  # v_bfe_u32(word, key, 1): offset = key[4:0]
            assert word < (1 << kb) // 32 and word * 32 + bit == key


def test_pass_rule_rewritten():
    """found + ~u >= sets (u = shared mismatches + ~bound as a signed word, negative for a survivor)  <=>  u - found < -sets;
    a lane that did not survive the zone level (u >= 0) never passes the second form"""
    for sets in (2, 3):
        for bound in range(0, 65):
            for k in range(0, 66):
                u = (k + (~bound & M32)) & M32
                signed = u - (1 << 32) if u >> 31 else u
                for found in range(sets + 1):
                    if signed < 0:
                        old = ((found + (~u & M32)) & M32) >= sets
                        assert (signed - found < -sets) == old, (sets, bound, k, found)
                        assert old == (found + (bound - k) >= sets)
                    else:
                        assert not (signed < -sets)

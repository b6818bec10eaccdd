"""GPU parity of both forms of the key test of scan_zone_kernel<.., DIRECT> in ONE launch (kernels.hip.h: kHoist, key_hoist).

A wave whose tile slots share no key column takes the hoisted form (keys from the query's own filter words, once per chunk);
a wave with a tile that shares one takes the per-tile form (keys with the tile's shared bits substituted).  The store here has
both kinds of wave, and the test proves that on the CPU before it scans.  It is packed with SMAFA_LAYOUT=0 (columns in file
order, a code table that does not depend on the rows), so the filter bit of every letter is known here from the file's table:

  * 2^20 + 100 uniform rows: a 256-row tile of the sorted store shares only leading columns of filter word 0;
  * TWIN, 1024 identical rows: equal rows have equal sort keys, so they are consecutive in the sorted store, and any 1024
    consecutive rows cover at least 3 whole tiles, which share EVERY column (all-ones masks);
  * PART, 1024 different rows with the same filter bits on columns 0..17 and on every key column (Y = 20..31, X and Z in
    word 1), free on columns 18, 19 and behind the key columns of word 1.  No other row of the store has their bits on
    columns 0..17 (such uniform rows are drawn again), and the sort keeps a common leading prefix together, so the block is
    consecutive: >= 3 whole tiles share all key columns with masks that are NOT all ones;
  * W1, 1024 different rows with the same filter bits on columns 0..19 (again theirs alone) and on word 1's key columns, half
    of them with some bits A on Y and half with ~A: the tile that holds both halves shares key columns of word 1 ONLY.

The zone words come from the host packer (`makedb_packed(.., device=-1)`: layout, stable sort and zone words restated with
plain loops, no GPU) of the rows generated here; from them the flag of every wave's tile group is evaluated as the kernel
evaluates it.  The test FAILS if a kind of wave or of tile named above is missing, or if no tile group mixes key-sharing tiles
with tiles that share no key column.  The packed file is then loaded and scanned, byte for byte against the oracle, with the
key test on every (chunk, tile) (SMAFA_ZONE_KEY_GATE=0), at the default gate and off.  Queries are planted next to all four
populations.
"""
import os
import struct

import numpy as np
import pytest

import oracle
import smafa_amd
from smafa_amd import synth

pytestmark = pytest.mark.gpu
BOUND = 5
# Copies of kernels.hip.h's defaults — SMAFA_ZONE_KEY_BITS and zone_tiles() of the two-word DIRECT kernels (the library does not
# export them).  If either default moves, move these with it: the proof below describes the kernel only while they agree.
KB = 12
TILES_PER_WAVE = {smafa_amd.ALPHABET_NT: 4, smafa_amd.ALPHABET_AA: 2}
N_LETTERS = {smafa_amd.ALPHABET_NT: 4, smafa_amd.ALPHABET_AA: 20}
N_ROWS = (1 << 20) + 100


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    oracle.build()
    assert smafa_amd.device_count() >= 1


def letter_codes(alphabet):
    """code bytes of the letters the rows are drawn from"""
    return synth.letter_codes(alphabet)[: N_LETTERS[alphabet]]


def key_columns(L):
    """(Y, X | Z) as masks of filter word 0 / word 1 (engine.hip launch_tiles: key_xmask, key_zlo; Y = word 0's last KB bits)"""
    n1 = min(L - 32, 32)
    xw = KB if n1 >= 2 * KB else n1 // 2
    cols1 = (1 << n1) - 1
    return (0xFFFFFFFF << (32 - KB)) & 0xFFFFFFFF, (((1 << xw) - 1) | (((1 << KB) - 1) << xw)) & cols1


def pack_on_host(path_fa, path_packed, rows, alphabet):
    """packed on the host with the fixed layout: no GPU involved in the proof"""
    synth.write_fasta(path_fa, rows, alphabet)
    old = os.environ.get("SMAFA_LAYOUT")
    os.environ["SMAFA_LAYOUT"] = "0"
    try:
        smafa_amd.makedb_packed(path_fa, path_packed, alphabet, device=-1)
    finally:
        if old is None:
            os.environ.pop("SMAFA_LAYOUT")
        else:
            os.environ["SMAFA_LAYOUT"] = old
    os.remove(path_fa)


def read_packed(path, L):
    """(perm, tab, zone words {c0, m0, c1, m1} per tile) of a packed store file"""
    raw = open(path, "rb").read()
    n_tiles = struct.unpack_from("<Q", raw, 8 + 24)[0]
    off_perm, off_tab = struct.unpack_from("<QQ", raw, 8 + 40)
    off_zone = struct.unpack_from("<Q", raw, 8 + 40 + 40)[0]
    perm = np.frombuffer(raw, dtype="<u4", count=L, offset=off_perm)
    tab = np.frombuffer(raw, dtype=np.uint8, count=L * 32, offset=off_tab).reshape(L, 32)
    zone = np.frombuffer(raw, dtype="<u4", count=4 * n_tiles, offset=off_zone).reshape(n_tiles, 4)
    return perm, tab, zone


def make_case(tmp_path, alphabet, L, seed):
    rng = np.random.default_rng(seed)
    lc = letter_codes(alphabet)
    # the fixed layout's table, from a small store of the same shape: filter bit of code v in column c = tab[c, v] & 1
    small = str(tmp_path / "small.packed")
    pack_on_host(str(tmp_path / "small.fa"), small, lc[rng.integers(0, len(lc), size=(4096, L))], alphabet)
    perm, tab, _ = read_packed(small, L)
    assert (perm == np.arange(L)).all()
    side = (tab[0, lc] & 1).astype(bool)  # per letter; the same in every column under this layout
    assert all(((tab[c, lc] & 1).astype(bool) == side).all() for c in range(L)) and side.any() and not side.all()
    letters = {0: lc[~side], 1: lc[side]}

    def fbits(rows):
        return side[np.searchsorted(lc, rows)] if (np.diff(lc) > 0).all() else None

    def rows_with_bits(bits, n):
        """n rows of random letters whose filter bits are `bits` (-1: any letter)"""
        out = lc[rng.integers(0, len(lc), size=(n, L))]
        for c in range(L):
            if bits[c] >= 0:
                pool = letters[int(bits[c])]
                out[:, c] = pool[rng.integers(0, len(pool), size=n)]
        return out

    ymask, xzmask = key_columns(L)
    key_cols = [c for c in range(32) if ymask >> c & 1] + [32 + c for c in range(32) if xzmask >> c & 1]
    s = lc[rng.integers(0, len(lc), size=(N_ROWS, L))]
    twin = lc[rng.integers(0, len(lc), size=L)]
    part_bits = np.full(L, -1)
    part_bits[list(range(18)) + key_cols] = rng.integers(0, 2, size=18 + len(key_cols))
    w1_bits = np.full(L, -1)
    w1_bits[list(range(20)) + [c for c in key_cols if c >= 32]] = rng.integers(0, 2, size=20 + sum(c >= 32 for c in key_cols))
    y_a = rng.integers(0, 2, size=KB)
    fb_twin = fbits(twin[None, :])[0]
    assert (fb_twin[:18] != part_bits[:18]).any() and (fb_twin[:20] != w1_bits[:20]).any() and (part_bits[:18] != w1_bits[:18]).any()
    while True:  # uniform rows inside PART's or W1's leading prefix are drawn again: the blocks then sort as one run each
        fb = fbits(s)
        inside = (fb[:, :18] == part_bits[:18]).all(axis=1) | (fb[:, :20] == w1_bits[:20]).all(axis=1)
        if not inside.any():
            break
        s[inside] = lc[rng.integers(0, len(lc), size=(int(inside.sum()), L))]
    part = rows_with_bits(part_bits, 1024)
    lo, hi = w1_bits.copy(), w1_bits.copy()
    lo[20:32], hi[20:32] = y_a, 1 - y_a
    w1 = np.r_[rows_with_bits(lo, 512), rows_with_bits(hi, 512)]
    where = rng.choice(N_ROWS, size=3072, replace=False)
    s[where[:1024]], s[where[1024:2048]], s[where[2048:]] = twin, part, w1
    q = []
    for i in range(96):  # next to the three blocks: exactly at the bound and one past it
        r = (twin, part[i], w1[(i * 37) % 1024])[i % 3].copy()
        for c in rng.choice(L, size=BOUND + (i & 1), replace=False):
            r[c] = lc[(np.searchsorted(lc, r[c]) + rng.integers(1, len(lc))) % len(lc)]
        q.append(r)
    for i in range(112):  # next to uniform rows: a few substitutions away
        r = s[rng.integers(0, N_ROWS)].copy()
        for c in rng.choice(L, size=int(rng.integers(0, BOUND + 2)), replace=False):
            r[c] = lc[(np.searchsorted(lc, r[c]) + rng.integers(1, len(lc))) % len(lc)]
        q.append(r)
    q += list(lc[rng.integers(0, len(lc), size=(16, L))])  # far rows
    return s, np.array(q, dtype=np.uint8), (perm, tab)


def scan(path, q, gate):
    old = os.environ.get("SMAFA_ZONE_KEY_GATE")
    if gate is None:
        os.environ.pop("SMAFA_ZONE_KEY_GATE", None)
    else:
        os.environ["SMAFA_ZONE_KEY_GATE"] = gate  # read when the handle is created
    try:
        store = smafa_amd.SubjectStore.load(path)
    finally:
        if old is None:
            os.environ.pop("SMAFA_ZONE_KEY_GATE", None)
        else:
            os.environ["SMAFA_ZONE_KEY_GATE"] = old
    try:
        store.set_zone_level(2)
        got = store.scan(q, max_divergence=BOUND)
        kernel = store.last_scan_kernel()
    finally:
        store.close()
    assert kernel.startswith("smafa::scan_zone_kernel") and kernel.endswith("2, true, true>"), kernel
    return got


def prove_both_forms(zone, alphabet, L):
    """from the host-packed zone words of the rows generated above: every kind of tile and of wave the docstring names"""
    assert len(zone) == (N_ROWS + 255) // 256
    ymask, xzmask = key_columns(L)
    cols1 = (1 << min(L - 32, 32)) - 1
    zm0, zm1 = zone[:, 1].astype(np.int64), zone[:, 3].astype(np.int64)
    shares = ((zm0 & ymask) != 0) | ((zm1 & xzmask) != 0)  # the kernel's flag, per tile
    all_ones = (zm0 == 0xFFFFFFFF) & (zm1 == cols1)
    all_keys = ((zm0 & ymask) == ymask) & ((zm1 & xzmask) == xzmask)
    kinds = {
        "identical rows (all-ones masks)": int(all_ones.sum()),
        "every key column shared, masks not all ones": int((all_keys & ~all_ones).sum()),
        "only key columns of word 1 shared": int((((zm0 & ymask) == 0) & ((zm1 & xzmask) != 0)).sum()),
    }
    assert kinds["identical rows (all-ones masks)"] >= 3, kinds
    assert kinds["every key column shared, masks not all ones"] >= 1, kinds  # (a whole tile inside one (18, 19) group of PART is all ones)
    assert kinds["only key columns of word 1 shared"] >= 1, kinds
    T = TILES_PER_WAVE[alphabet]
    pad = (-len(shares)) % T  # tile slots past the range: zone words 0
    groups = np.r_[shares, np.zeros(pad, dtype=bool)].reshape(-1, T)
    waves = {
        "hoisted": int((~groups.any(axis=1)).sum()),
        "per-tile": int(groups.any(axis=1).sum()),
        "per-tile with a tile that shares no key column": int((groups.any(axis=1) & ~groups.all(axis=1)).sum()),
    }
    assert waves["hoisted"] >= len(groups) // 2, waves  # the uniform rows
    assert waves["per-tile"] >= 3, waves  # at least one per planted block
    assert waves["per-tile with a tile that shares no key column"] >= 1, waves  # both kinds of tile in one wave's tile group
    return kinds, waves


CASES = [(smafa_amd.ALPHABET_AA, L) for L in (33, 44, 56, 60, 64)] + [(smafa_amd.ALPHABET_NT, L) for L in (33, 60)]


@pytest.mark.parametrize("alphabet,L", CASES)
def test_both_forms_in_one_launch_match_oracle(tmp_path, alphabet, L):
    s, q, (perm, tab) = make_case(tmp_path, alphabet, L, 2000 * alphabet + L)
    packed = str(tmp_path / "s.packed")
    pack_on_host(str(tmp_path / "s.fa"), packed, s, alphabet)
    perm2, tab2, zone = read_packed(packed, L)
    assert (perm2 == perm).all() and (tab2 == tab).all()  # the layout the rows were built for
    kinds, waves = prove_both_forms(zone, alphabet, L)
    print("L=%d alphabet=%d: tiles %s, waves %s" % (L, alphabet, kinds, waves))
    want = oracle.scan_codes(s, q, BOUND)
    # the planted queries: hits at the bound for the even ones of every block, and next to the uniform rows
    for block in range(3):
        near = np.arange(block, 96, 3)
        assert len(np.intersect1d(want["query"], near[near % 2 == 0])) == 16, block
    assert len(np.unique(want["query"][(want["query"] >= 96) & (want["query"] < 208)])) >= 56
    for gate in ("0", None, "65"):  # the key test forced on, at the default gate, off
        assert scan(packed, q, gate).tobytes() == want.tobytes(), gate

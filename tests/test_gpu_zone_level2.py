"""GPU parity of level 2 of scan_zone_kernel<.., DIRECT> on two-word stores (kernels.hip.h: kL2Lanes, zone_f1_home).

Level 2 folds the filter plane over both its words.  In the key-test kernels the query's filter word 1 comes out of lane i of the
chunk's heads and the tile's filter word 1 from where the prologue left it (LDS or L2, per shape); the query record is
read only for level 3.  The queries here are built, on the CPU, to stop at each of those levels next to known subjects:

  (a) filter word 0 as the subject's, BOUND + 1 filter-bit flips in word 1                : passes level 1, rejected at level 2
  (b) the same with exactly BOUND flips                                                   : a row at distance BOUND
  (c) BOUND + 1 substitutions in word 1 that keep the filter bit                          : passes level 2, rejected at level 3

(where word 1 has fewer than BOUND + 1 columns, L = 33, the flips that do not fit go to word 0: level 1 still passes, since at
most BOUND of them are there).  The subjects they stand next to lie in tile slot 0 of a wave, in the slots behind it and in the
last live slot of the last wave, whose other slots are dead: the tile count is no multiple of the tiles per wave, which the test
takes from `last_scan_plan()` and asserts.  Stores are packed on the host with SMAFA_LAYOUT=0 (columns in file order, a code table
that does not depend on the rows), so the filter bit of every letter is known here, and the classes are counted from those bits
before anything is scanned.  A block of identical rows gives waves that take the per-tile form of the key test next to the
uniform rows' waves, which take the hoisted form; both are proven from the host-packed zone words for the kernel's own tile
grouping.  Rows are compared byte for byte with the oracle at SMAFA_ZONE_KEY_GATE=0 (always test), the default and 65 (never).

The dense case plants a family of 400 near copies and a first chunk of queries next to all of them, so the family's wave leaves
the prefilter for the register-resident walk (proven from the sorted order: two family tiles in one wave), walks 15 chunks and
probes again at chunk 16 — where queries of the three classes wait next to the family.  Whatever the prologue left in registers
has to be there again after the walk.
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
KB = 12  # kernels.hip.h: SMAFA_ZONE_KEY_BITS (the library does not export it)
N_LETTERS = {smafa_amd.ALPHABET_NT: 4, smafa_amd.ALPHABET_AA: 20}
N_SMALL = 20_020  # 78 whole tiles and one of 52 rows
N_LARGE = (1 << 20) + 100
TWIN = 600  # identical rows: consecutive in the sorted store, at least one whole tile
PER_CLASS = 8  # queries per (planted tile, class)


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    oracle.build()
    assert smafa_amd.device_count() >= 1


def key_columns(L):
    """(Y, X | Z) as masks of filter word 0 / word 1 (engine.hip launch_tiles: key_xmask, key_zlo; Y = word 0's last KB bits)"""
    n1 = min(L - 32, 32)
    xw = KB if n1 >= 2 * KB else n1 // 2
    cols1 = (1 << n1) - 1
    return (0xFFFFFFFF << (32 - KB)) & 0xFFFFFFFF, (((1 << xw) - 1) | (((1 << KB) - 1) << xw)) & cols1


def pack_on_host(path_fa, path_packed, rows, alphabet):
    """packed on the host with the fixed layout: no GPU involved in what the test proves before it scans"""
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
    """(perm, tab, order: sorted position -> subject, zone words {c0, m0, c1, m1} per tile) of a packed store file"""
    raw = open(path, "rb").read()
    n, n_tiles = struct.unpack_from("<QQ", raw, 8 + 16)
    off_perm, off_tab = struct.unpack_from("<QQ", raw, 8 + 40)
    off_order, off_zone = struct.unpack_from("<QQ", raw, 8 + 40 + 32)
    perm = np.frombuffer(raw, dtype="<u4", count=L, offset=off_perm)
    tab = np.frombuffer(raw, dtype=np.uint8, count=L * 32, offset=off_tab).reshape(L, 32)
    order = np.frombuffer(raw, dtype="<u4", count=n, offset=off_order)
    zone = np.frombuffer(raw, dtype="<u4", count=4 * n_tiles, offset=off_zone).reshape(n_tiles, 4)
    assert n_tiles == (n + 255) // 256 and (np.sort(order) == np.arange(n)).all()
    return perm, tab, order, zone


class Letters:
    """the letters of an alphabet and the side of the filter bit each is on, from the fixed layout's code table"""

    def __init__(self, tmp_path, alphabet, L, rng):
        self.lc = synth.letter_codes(alphabet)[: N_LETTERS[alphabet]]
        assert (np.diff(self.lc) > 0).all()
        small = str(tmp_path / "small.packed")
        pack_on_host(str(tmp_path / "small.fa"), small, self.lc[rng.integers(0, len(self.lc), size=(4096, L))], alphabet)
        self.perm, self.tab, _, _ = read_packed(small, L)
        assert (self.perm == np.arange(L)).all()
        self.side = (self.tab[0, self.lc] & 1).astype(bool)  # per letter; the same in every column under this layout
        assert all(((self.tab[c, self.lc] & 1).astype(bool) == self.side).all() for c in range(L))
        assert self.side.sum() >= 2 and (~self.side).sum() >= 2  # a flip and a bit-keeping substitution exist for every letter

    def fbits(self, rows):
        return self.side[np.searchsorted(self.lc, rows)]

    def substitute(self, rng, letter, flip):
        """another letter, on the other side of the filter bit (flip) or on the same side"""
        mine = self.side[np.searchsorted(self.lc, letter)]
        pool = self.lc[(self.side != mine) if flip else ((self.side == mine) & (self.lc != letter))]
        return pool[rng.integers(0, len(pool))]

    def random_sub(self, rng, letter):
        return self.lc[(np.searchsorted(self.lc, letter) + rng.integers(1, len(self.lc))) % len(self.lc)]


def planted_query(rng, ab, subject, L, n_subs, flip):
    """`n_subs` substitutions, in word 1 as far as it has columns and in word 0 for the rest; flip: each changes the filter bit"""
    n1 = min(n_subs, L - 32)
    cols = np.r_[32 + rng.choice(L - 32, size=n1, replace=False), rng.choice(32, size=n_subs - n1, replace=False)].astype(int)
    r = subject.copy()
    for c in cols:
        r[c] = ab.substitute(rng, r[c], flip)
    return r


def classify(ab, query, subject):
    """the level at which the pair (query, subject) stops, from the filter bits: 'a' level 2, 'b' a row at BOUND, 'c' level 3"""
    fq, fs = ab.fbits(query), ab.fbits(subject)
    fd0, fd1 = int((fq[:32] != fs[:32]).sum()), int((fq[32:] != fs[32:]).sum())
    d = int((query != subject).sum())
    if fd0 <= BOUND and fd0 + fd1 == BOUND + 1:
        return "a"
    if fd0 + fd1 == BOUND and d == BOUND:
        return "b"
    if fd0 + fd1 == 0 and d == BOUND + 1:
        return "c"
    return "?"


def planted_classes(rng, ab, s, subjects, L):
    """PER_CLASS queries of each class next to subjects drawn from `subjects`: (queries, [(class, subject)])"""
    q, tags = [], []
    for cls, n_subs, flip in (("a", BOUND + 1, True), ("b", BOUND, True), ("c", BOUND + 1, False)):
        for subj in rng.choice(subjects, size=PER_CLASS, replace=len(subjects) < PER_CLASS):
            q.append(planted_query(rng, ab, s[subj], L, n_subs, flip))
            tags.append((cls, int(subj)))
    return q, tags


def check_classes(ab, s, q, tags, first, L):
    """the planted queries q[first:first + len(tags)] are of the class they were built for, counted from the filter bits"""
    seen = {"a": 0, "b": 0, "c": 0}
    for k, (cls, subj) in enumerate(tags):
        assert classify(ab, q[first + k], s[subj]) == cls, (k, cls)
        if cls == "a" and L - 32 >= BOUND + 1:
            assert (q[first + k][:32] == s[subj][:32]).all()  # word 0 identical
        seen[cls] += 1
    assert seen["a"] == seen["b"] == seen["c"] == len(tags) // 3 and seen["a"] >= PER_CLASS, seen
    return seen


def check_rows(want, tags, first):
    """the oracle agrees: a row at BOUND for every (b) pair, none for the (a) and (c) pairs"""
    rows = set(zip(want["query"].tolist(), want["subject"].tolist()))
    for k, (cls, subj) in enumerate(tags):
        assert ((first + k, subj) in rows) == (cls == "b"), (k, cls)


def scan(path, q, gate, query_block):
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
        store.set_query_block(query_block)
        got = store.scan(q, max_divergence=BOUND)
        kernel, plan = store.last_scan_kernel(), store.last_scan_plan()
    finally:
        store.close()
    assert kernel.startswith("smafa::scan_zone_kernel") and kernel.endswith("2, true, true>"), kernel
    return got, plan


def prove_wave_forms(zone, L, T, mostly_hoisted):
    """both forms of the key test run in this launch, for T tiles per wave: from the host-packed zone words"""
    ymask, xzmask = key_columns(L)
    shares = ((zone[:, 1].astype(np.int64) & ymask) != 0) | ((zone[:, 3].astype(np.int64) & xzmask) != 0)  # the kernel's flag, per tile
    groups = np.r_[shares, np.zeros((-len(shares)) % T, dtype=bool)].reshape(-1, T)  # tile slots past the range: zone words 0
    waves = {"hoisted": int((~groups.any(axis=1)).sum()), "per-tile": int(groups.any(axis=1).sum())}
    assert waves["hoisted"] >= (len(groups) // 2 if mostly_hoisted else 1) and waves["per-tile"] >= 1, waves
    return waves


def make_store(rng, ab, n_rows, L):
    s = ab.lc[rng.integers(0, len(ab.lc), size=(n_rows, L))]
    s[rng.choice(n_rows, size=TWIN, replace=False)] = ab.lc[rng.integers(0, len(ab.lc), size=L)]
    return s


CASES = [(smafa_amd.ALPHABET_AA, L, N_SMALL) for L in (33, 60, 64)] + [(smafa_amd.ALPHABET_NT, L, N_SMALL) for L in (33, 60)] + [
    (smafa_amd.ALPHABET_AA, 60, N_LARGE)]


@pytest.mark.parametrize("alphabet,L,n_rows", CASES)
def test_level2_classes_match_oracle(tmp_path, alphabet, L, n_rows):
    rng = np.random.default_rng(7000 * alphabet + 10 * L + (n_rows > N_SMALL))
    ab = Letters(tmp_path, alphabet, L, rng)
    s = make_store(rng, ab, n_rows, L)
    packed = str(tmp_path / "s.packed")
    pack_on_host(str(tmp_path / "s.fa"), packed, s, alphabet)
    perm, tab, order, zone = read_packed(packed, L)
    assert (perm == ab.perm).all() and (tab == ab.tab).all()  # the layout the filter bits were read from
    n_tiles = len(zone)
    # next to subjects of tiles 0..3 (slot 0 and the slots behind it, whatever the tiles per wave) and of the last tile
    planted_tiles = [0, 1, 2, 3, n_tiles - 1]
    q, tags = [], []
    for tile in planted_tiles:
        qs, ts = planted_classes(rng, ab, s, order[tile * 256 : min((tile + 1) * 256, n_rows)], L)
        q += qs
        tags += [(cls, subj, tile) for cls, subj in ts]
    n_planted = len(q)
    for _ in range(80):  # next to uniform rows: a few substitutions away
        r = s[rng.integers(0, n_rows)].copy()
        for c in rng.choice(L, size=int(rng.integers(0, BOUND + 2)), replace=False):
            r[c] = ab.random_sub(rng, r[c])
        q.append(r)
    q += list(ab.lc[rng.integers(0, len(ab.lc), size=(16, L))])  # far rows
    q = np.array(q, dtype=np.uint8)
    seen = check_classes(ab, s, q, [(c, sj) for c, sj, _ in tags], 0, L)
    assert seen["a"] == PER_CLASS * len(planted_tiles)
    want = oracle.scan_codes(s, q, BOUND)
    check_rows(want, [(c, sj) for c, sj, _ in tags], 0)
    assert n_planted > 96  # planted queries in chunk 0 of block 0, in its short chunk and in block 1
    for gate in ("0", None, "65"):  # the key test on every chunk, at the default gate, off
        got, plan = scan(packed, q, gate, 96)
        T = plan["tiles_per_wave"]
        assert plan["query_blocks"] >= 2 and 96 % 64 != 0  # blocks end mid-chunk
        assert n_tiles % T != 0  # the last wave has dead tile slots
        slots = {tile % T for _, _, tile in tags}
        assert 0 in slots and T - 1 in slots and (n_tiles - 1) % T in slots, (T, slots)
        waves = prove_wave_forms(zone, L, T, mostly_hoisted=n_rows > N_SMALL)
        print("L=%d alphabet=%d rows=%d gate=%s: T=%d, waves %s, classes %s" % (L, alphabet, n_rows, gate, T, waves, seen))
        assert got.tobytes() == want.tobytes(), gate


def make_dense_case(tmp_path, alphabet, L, seed):
    rng = np.random.default_rng(seed)
    ab = Letters(tmp_path, alphabet, L, rng)
    s = make_store(rng, ab, N_SMALL, L)
    base = ab.lc[rng.integers(0, len(ab.lc), size=L)]
    family = np.tile(base, (400, 1))
    for r in family:  # near copies: 1..3 substitutions in word 1, so the family shares word 0 and sorts as one run
        for c in 32 + rng.choice(L - 32, size=int(rng.integers(1, 4)), replace=False):
            r[c] = ab.random_sub(rng, r[c])
    while True:  # no other row inside the family's run
        inside = (ab.fbits(s[:, :32]) == ab.fbits(base[:32])).all(axis=1)
        if not inside.any():
            break
        s[inside] = ab.lc[rng.integers(0, len(ab.lc), size=(int(inside.sum()), L))]
    members = rng.choice(N_SMALL, size=400, replace=False)
    s[members] = family
    return rng, ab, s, base, members


def test_dense_walk_and_back(tmp_path):
    alphabet, L = smafa_amd.ALPHABET_AA, 60
    # (this seed's family lies in three consecutive tiles: two of them share a wave whether a wave takes 2, 3 or 4 tiles)
    rng, ab, s, base, members = make_dense_case(tmp_path, alphabet, L, 4244)
    packed = str(tmp_path / "s.packed")
    pack_on_host(str(tmp_path / "s.fa"), packed, s, alphabet)
    perm, tab, order, zone = read_packed(packed, L)
    assert (perm == ab.perm).all() and (tab == ab.tab).all()
    pos = np.empty(N_SMALL, dtype=np.int64)
    pos[order] = np.arange(N_SMALL)
    family_tiles = np.unique(pos[members] // 256)
    assert family_tiles[-1] - family_tiles[0] == len(family_tiles) - 1 and len(family_tiles) in (2, 3)  # one run
    q = []
    for _ in range(64):  # chunk 0: one substitution from the base, within BOUND of every member, so every family tile passes level 3
        r = base.copy()
        c = 32 + rng.integers(0, L - 32)
        r[c] = ab.random_sub(rng, r[c])
        q.append(r)
    assert all(int((r != s[m]).sum()) <= BOUND for r in q[:8] for m in members)
    for _ in range(15 * 64 - 4 * 3 * PER_CLASS):  # chunks 1..15, walked densely by the family's wave: far rows and rows near uniform subjects
        r = s[rng.integers(0, N_SMALL)].copy()
        for c in rng.choice(L, size=int(rng.integers(0, BOUND + 2)), replace=False):
            r[c] = ab.random_sub(rng, r[c])
        q.append(r)
    first_walk = len(q)
    qs_walk, tags_walk = [], []
    for _ in range(4):  # ... and 4 x 3 x PER_CLASS of the three classes next to the family (the walk compares exactly)
        qs, ts = planted_classes(rng, ab, s, members, L)
        qs_walk += qs
        tags_walk += ts
    q += qs_walk
    assert len(q) == 16 * 64
    # chunk 16 and on: the wave probes the prefilter again — the three classes next to the family and next to the other subjects
    # of its tiles, among far rows
    first_back = len(q)
    neighbours = np.setdiff1d(order[family_tiles[0] * 256 : min((family_tiles[-1] + 1) * 256, N_SMALL)], members)
    tags_back = []
    for pool in (members, neighbours, members, neighbours):
        if len(pool) == 0:
            pool = members
        qs, ts = planted_classes(rng, ab, s, pool, L)
        q += qs
        tags_back += ts
    q += list(ab.lc[rng.integers(0, len(ab.lc), size=(3 * 64 - len(tags_back), L))])
    q = np.array(q, dtype=np.uint8)
    assert len(q) == 19 * 64
    check_classes(ab, s, q, tags_walk, first_walk, L)
    check_classes(ab, s, q, tags_back, first_back, L)
    want = oracle.scan_codes(s, q, BOUND)
    check_rows(want, tags_walk, first_walk)
    check_rows(want, tags_back, first_back)
    for gate in ("0", None, "65"):
        got, plan = scan(packed, q, gate, 2048)  # one block of 19 chunks: the walk starts behind chunk 0 and ends in front of chunk 16
        T = plan["tiles_per_wave"]
        assert plan["query_blocks"] == 1
        # a wave leaves the prefilter behind a chunk with passes * 5 > 64 * 8 (kernels.hip.h), passes = its (query, tile) pairs that
        # reached level 3: chunk 0 gives 64 per family tile, so a wave that holds two family tiles walks densely
        per_wave = np.bincount(family_tiles // T)
        assert per_wave.max() >= 2 and 64 * per_wave.max() * 5 > 64 * 8, (T, family_tiles)
        assert got.tobytes() == want.tobytes(), gate

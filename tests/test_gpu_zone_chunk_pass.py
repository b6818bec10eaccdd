"""GPU parity of the chunk loops of scan_zone_kernel<.., DIRECT> on two-word stores (kernels.hip.h: chunk_pass, kSplit).

The key-test kernels classify each wave once.  A *plain* wave — inside the range with all its tile slots, no slot shares a key
column, none shares a column of filter word 1 — runs the chunk body with those facts compiled in; every other wave runs the
general body.  Either body comes in two forms: a full chunk (64 live queries, no lane mask, the next chunk's heads fetched
unconditionally) and the last chunk of a query block (1..64 live queries; its other lanes hold the next block's heads or the
zero records behind the last query).  What can go wrong lies at the edges of that split, and every case here plants rows there:

  * query counts 65, 128, 129 and 64 * 17 + 1 under the automatic block size, and 64 * 17 + 1 under block sizes that end a block in
    a chunk of 1, of 63 and of exactly 64 live queries, and one block of 18 chunks.  Counts 1, 63 and 64 are scanned too, but the
    host serves up to 64 queries with scan_zone_few_kernel: they run none of the code this file is about (the name is asserted
    either way), and chunks of 1, 63 and 64 live queries reach the DIRECT kernel only as the last chunk of a block; hits for the last live query of a tail chunk,
    for the first query of the next block (reported once, by its own block) and for the last query of the whole set;
  * a store with 1024 identical rows among uniform ones and 257 tiles: plain and general waves in one launch, the last wave with
    one live slot — both kinds proven on the CPU from the host packer's zone words, for the kernel's own tile grouping; hits in
    the first tile, in slot 1 of a plain wave, in a general wave and in the last wave's only live slot;
  * 18 chunks of queries next to a dense family (the waves that hold it leave the prefilter and come back), followed by 18 chunks
    of far queries in the same block; the same launch with the two halves in the other order returns the same rows;
  * a one-tile store and a store of exactly T tiles.

Rows are compared byte for byte with the oracle at SMAFA_ZONE_KEY_GATE=0 (always test), the default and 65 (never), and the
oracle's rows are checked, before anything is scanned, to hold every planted pair.
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
N_ROWS = (1 << 16) + 100  # 257 tiles: odd, and 1 past a multiple of 4 — the last wave has one live slot at 2 and at 4 tiles per wave
TWIN = 1024  # identical rows: consecutive in the sorted store, at least 3 whole tiles with all-ones zone masks
GATES = ("0", None, "65")
# (alphabet, row length, letters drawn from, kernel name starts with)
SHAPES = {
    "aa60": (smafa_amd.ALPHABET_AA, 60, 20, "smafa::scan_zone_kernel<5, 5, 2, true, true>"),
    "aa33": (smafa_amd.ALPHABET_AA, 33, 20, "smafa::scan_zone_kernel<5, 5, 2, true, true>"),
    "nt60": (smafa_amd.ALPHABET_NT, 60, 4, "smafa::scan_zone_kernel<2, 3, 2, true, true>"),
    "ntN60": (smafa_amd.ALPHABET_NT, 60, 5, "smafa::scan_zone_kernel<3, 3, 2, true, true>"),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    oracle.build()
    assert smafa_amd.device_count() >= 1


def letters_of(shape):
    alphabet, _, n_letters, _ = SHAPES[shape]
    lc = synth.letter_codes(alphabet)
    if n_letters > len(lc):  # nucleotides with N (code 4): the three-plane store
        lc = np.r_[lc, np.uint8(4)].astype(np.uint8)
    return lc[:n_letters]


def key_columns(L):
    """(Y, X | Z) as masks of filter word 0 / word 1 (engine.hip launch_tiles: key_xmask, key_zlo; Y = word 0's last KB bits)"""
    n1 = min(L - 32, 32)
    xw = KB if n1 >= 2 * KB else n1 // 2
    cols1 = (1 << n1) - 1
    return (0xFFFFFFFF << (32 - KB)) & 0xFFFFFFFF, (((1 << xw) - 1) | (((1 << KB) - 1) << xw)) & cols1


def pack_on_host(tmp_path, rows, alphabet):
    """the store packed by the host packer (no GPU): -> (path, order: sorted position -> subject, zone words per tile)"""
    fa, packed = str(tmp_path / "s.fa"), str(tmp_path / ("s%d.packed" % len(os.listdir(tmp_path))))
    synth.write_fasta(fa, rows, alphabet)
    smafa_amd.makedb_packed(fa, packed, alphabet, device=-1)
    os.remove(fa)
    raw = open(packed, "rb").read()
    n, n_tiles = struct.unpack_from("<QQ", raw, 8 + 16)
    off_order, off_zone = struct.unpack_from("<QQ", raw, 8 + 40 + 32)
    order = np.frombuffer(raw, dtype="<u4", count=n, offset=off_order)
    zone = np.frombuffer(raw, dtype="<u4", count=4 * n_tiles, offset=off_zone).reshape(n_tiles, 4)
    assert n == len(rows) and n_tiles == (n + 255) // 256 and (np.sort(order) == np.arange(n)).all()
    return packed, order, zone


def wave_kinds(zone, L, T):
    """per wave (T consecutive tiles), as the kernel's prologue decides it: True = plain"""
    ymask, xzmask = key_columns(L)
    m0, m1 = zone[:, 1].astype(np.int64), zone[:, 3].astype(np.int64)
    odd = ((m0 & ymask) != 0) | ((m1 & xzmask) != 0) | (m1 != 0)  # shares a key column, or any column of word 1
    pad = (-len(zone)) % T
    groups = np.r_[odd, np.zeros(pad, dtype=bool)].reshape(-1, T)
    plain = ~groups.any(axis=1)
    if pad:
        plain[-1] = False  # dead tile slots
    return plain


def mutate(rng, lc, row, n_subs):
    r = row.copy()
    for c in rng.choice(len(r), size=n_subs, replace=False):
        r[c] = lc[(np.searchsorted(lc, r[c]) + rng.integers(1, len(lc))) % len(lc)]
    return r


def far_queries(rng, lc, n, L):
    return lc[rng.integers(0, len(lc), size=(n, L))]


class Handle:
    """a store loaded under a key gate (read when the handle is created)"""

    def __init__(self, packed, gate):
        old = os.environ.get("SMAFA_ZONE_KEY_GATE")
        if gate is None:
            os.environ.pop("SMAFA_ZONE_KEY_GATE", None)
        else:
            os.environ["SMAFA_ZONE_KEY_GATE"] = gate
        try:
            self.store = smafa_amd.SubjectStore.load(packed)
        finally:
            if old is None:
                os.environ.pop("SMAFA_ZONE_KEY_GATE", None)
            else:
                os.environ["SMAFA_ZONE_KEY_GATE"] = old
        self.store.set_zone_level(2)

    def scan(self, q, query_block, kernel):
        self.store.set_query_block(query_block)  # 0: the automatic size
        got = self.store.scan(q, max_divergence=BOUND)
        # (up to 64 queries the host launches scan_zone_few_kernel instead: those counts are checked against the oracle all the same,
        # and chunks of 1, 63 and 64 live queries reach the DIRECT kernel as the last chunk of a block)
        want = kernel if len(q) > 64 else "smafa::scan_zone_few_kernel"
        assert self.store.last_scan_kernel().startswith(want), self.store.last_scan_kernel()
        return got, self.store.last_scan_plan()

    def close(self):
        self.store.close()


def mixed_store(rng, lc, L):
    s = lc[rng.integers(0, len(lc), size=(N_ROWS, L))]
    s[rng.choice(N_ROWS, size=TWIN, replace=False)] = lc[rng.integers(0, len(lc), size=L)]
    return s


def tiles_per_wave(packed, lc, L, kernel):
    h = Handle(packed, None)
    try:
        _, plan = h.scan(far_queries(np.random.default_rng(1), lc, 65, L), 0, kernel)
    finally:
        h.close()
    return plan["tiles_per_wave"]


def planted_tiles(zone, L, T):
    """[first tile, slot 1 of a plain wave, a tile of a general wave inside the range, the last wave's only live slot]"""
    plain = wave_kinds(zone, L, T)
    n_tiles = len(zone)
    assert n_tiles % T == 1  # the last wave has one live slot
    inside = np.arange(len(plain)) < n_tiles // T
    assert (plain & inside).sum() >= 8 and (~plain & inside).sum() >= 1, (plain.sum(), len(plain))  # both kinds of wave
    w_plain = int(np.nonzero(plain & inside)[0][3])
    w_general = int(np.nonzero(~plain & inside)[0][0])
    return [0, w_plain * T + 1, w_general * T, n_tiles - 1], plain


def plant(rng, lc, s, order, tiles, q, at):
    """q[at[k]] becomes a near copy of a subject of tiles[k % len(tiles)]: -> [(query, subject)]"""
    pairs = []
    for k, i in enumerate(at):
        tile = tiles[k % len(tiles)]
        subj = int(rng.choice(order[tile * 256 : min((tile + 1) * 256, len(s))]))
        q[i] = mutate(rng, lc, s[subj], int(rng.integers(0, BOUND + 1)))
        pairs.append((int(i), subj))
    return pairs


def check_planted(want, pairs):
    """the oracle alone reports every planted pair: a case in which nothing can hit hides nothing"""
    rows = set(zip(want["query"].tolist(), want["subject"].tolist()))
    assert len(want) > 0 and all(p in rows for p in pairs), [p for p in pairs if p not in rows]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_chunk_and_block_edges(tmp_path, shape):
    alphabet, L, _, kernel = SHAPES[shape]
    lc = letters_of(shape)
    rng = np.random.default_rng(2700 + 7 * L + len(lc))
    s = mixed_store(rng, lc, L)
    packed, order, zone = pack_on_host(tmp_path, s, alphabet)
    T = tiles_per_wave(packed, lc, L, kernel)
    tiles, plain = planted_tiles(zone, L, T)
    print("%s: T=%d, %d plain waves, %d general, planted tiles %s" % (shape, T, plain.sum(), (~plain).sum(), tiles))
    # (query count, block size; 0 = automatic): blocks that end in a chunk of 1 (65), of 63 (127), of exactly 64 (128), and one block
    # of 18 chunks whose last holds one query (2048)
    runs = [(n, 0) for n in (1, 63, 64, 65, 128, 129, 64 * 17 + 1)] + [(64 * 17 + 1, qb) for qb in (65, 127, 128, 2048)]
    cases = {}
    for nq, qb in runs:
        q = far_queries(rng, lc, nq, L)
        at = {0, nq - 1, nq // 2}  # the first query, the last of the whole set (its chunk's other lanes read the array's padding)
        if qb:
            for b in range(1, min(4, (nq + qb - 1) // qb)):
                at |= {b * qb - 1, b * qb}  # the last live query of a block's tail chunk, the first query of the next block
        pairs = plant(rng, lc, s, order, tiles, q, sorted(i for i in at if 0 <= i < nq))
        want = oracle.scan_codes(s, q, BOUND)
        check_planted(want, pairs)
        cases[(nq, qb)] = (q, want)
    for gate in GATES:
        h = Handle(packed, gate)
        try:
            for (nq, qb), (q, want) in cases.items():
                got, plan = h.scan(q, qb, kernel)
                assert nq <= 64 or plan["tiles_per_wave"] == T
                if qb:
                    assert plan["query_blocks"] == (nq + qb - 1) // qb
                assert got.tobytes() == want.tobytes(), (shape, gate, nq, qb)
        finally:
            h.close()


def test_filter_off_and_back_on(tmp_path):
    shape = "aa60"
    alphabet, L, _, kernel = SHAPES[shape]
    lc = letters_of(shape)
    rng = np.random.default_rng(2727)
    s = mixed_store(rng, lc, L)
    # a dense family: 768 copies of one row with 2 or 3 substitutions each, all behind column 20 — the members share their leading
    # columns (one run of the sorted store) and, 256 to a tile, disagree on every key column and on every column of word 1
    base = lc[rng.integers(0, len(lc), size=L)]
    members = rng.choice(N_ROWS, size=768, replace=False)
    for m in members:
        s[m] = base
        s[m, 20:] = mutate(rng, lc, base[20:], int(rng.integers(2, 4)))
    packed, order, zone = pack_on_host(tmp_path, s, alphabet)
    T = tiles_per_wave(packed, lc, L, kernel)
    pos = np.empty(N_ROWS, dtype=np.int64)
    pos[order] = np.arange(N_ROWS)
    # `passes` counts the (query, tile) pairs of a chunk that reached the exact comparison: 64 per tile that holds a member, since
    # every query of `near` is within BOUND of every member.  A wave leaves the prefilter behind a chunk with passes * 5 > 64 * 8:
    # one that holds two family tiles or more.  The exit that is new is the PLAIN body's, so one such wave has to be plain.
    fam_tiles = np.unique(pos[members] // 256)
    tiles_in_wave = np.bincount(fam_tiles // T, minlength=(len(zone) + T - 1) // T)
    plain = wave_kinds(zone, L, T)
    tripping = (tiles_in_wave >= 2) & (64 * tiles_in_wave * 5 > 64 * 8)
    assert (tripping & plain).any(), (T, fam_tiles, np.nonzero(tripping)[0], plain[np.nonzero(tripping)[0]])
    n_half = 18 * 64
    near = np.array([mutate(rng, lc, base, 1) for _ in range(n_half)], dtype=np.uint8)
    assert all(int((near[i] != s[m]).sum()) <= BOUND for i in (0, 1, n_half - 1) for m in members[:64])
    far = far_queries(rng, lc, n_half, L)
    tiles, _ = planted_tiles(zone, L, T)
    pairs_far = plant(rng, lc, s, order, tiles + [int(fam_tiles[0])], far, [0, 1, 64, 16 * 64, 17 * 64 + 62, n_half - 1])
    q_ab, q_ba = np.r_[near, far], np.r_[far, near]
    want_ab, want_ba = oracle.scan_codes(s, q_ab, BOUND), oracle.scan_codes(s, q_ba, BOUND)
    check_planted(want_ab, [(n_half + i, sj) for i, sj in pairs_far] + [(0, int(members[0])), (n_half - 1, int(members[-1]))])
    check_planted(want_ba, pairs_far + [(n_half, int(members[0]))])
    # the same rows in either order, the query numbers moved by half
    moved = want_ba.copy()
    moved["query"] = (moved["query"] + n_half) % (2 * n_half)
    assert np.sort(moved, order=["query", "dist", "subject"]).tobytes() == want_ab.tobytes()
    for gate in GATES:
        h = Handle(packed, gate)
        try:
            got_ab, plan = h.scan(q_ab, 4096, kernel)  # one block of 36 chunks
            assert plan["query_blocks"] == 1
            got_ba, _ = h.scan(q_ba, 4096, kernel)
        finally:
            h.close()
        assert got_ab.tobytes() == want_ab.tobytes() and got_ba.tobytes() == want_ba.tobytes(), gate
        back = got_ba.copy()
        back["query"] = (back["query"] + n_half) % (2 * n_half)
        assert np.sort(back, order=["query", "dist", "subject"]).tobytes() == got_ab.tobytes(), gate


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n_tiles", ["one", "T"])
def test_tiny_stores(tmp_path, shape, n_tiles):
    alphabet, L, _, kernel = SHAPES[shape]
    lc = letters_of(shape)
    rng = np.random.default_rng(2750 + 7 * L + len(lc))
    probe, _, _ = pack_on_host(tmp_path, far_queries(rng, lc, 300, L), alphabet)
    T = tiles_per_wave(probe, lc, L, kernel)
    n_rows = 200 if n_tiles == "one" else 256 * T  # at most one tile; exactly T whole tiles: one wave, every slot live
    s = far_queries(rng, lc, n_rows, L)
    packed, order, zone = pack_on_host(tmp_path, s, alphabet)
    assert len(zone) == (1 if n_tiles == "one" else T)
    nq = 64 * 2 + 1
    q = far_queries(rng, lc, nq, L)
    pairs = plant(rng, lc, s, order, list(range(len(zone))), q, [0, 63, 64, 127, 128])
    want = oracle.scan_codes(s, q, BOUND)
    check_planted(want, pairs)
    for gate in GATES:
        h = Handle(packed, gate)
        try:
            for qb in (0, 65):
                got, _ = h.scan(q, qb, kernel)
                assert got.tobytes() == want.tobytes(), (shape, gate, qb)
        finally:
            h.close()

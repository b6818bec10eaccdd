"""The neighbours call's pipeline as a numpy model (CPU), held against brute force, and its key rule from the header compiled
for the host.

The model does what smafa_db_self_neighbours_launch does behind the join (neighbours.hip.h, self_join.hip.h: join_neighbours):
every pair arrives ONCE, in an arbitrary order and orientation; it is packed as two entries; the entries are sorted — as one
64-bit key, row << (32 + dist_bits) | dist << 32 | neighbour, or by two stable sorts with the row apart —; lower[i] is a
binary search per row; with a cut the degrees are cut and summed; every entry of rank < k leaves for offsets[row] + rank.
The expected answers are tests/neighbours_cases.py::brute_neighbours, which works row by row on the code bytes and shares
no step with the model.  The key rule's expected values are worked by hand from its definition: dist_bits = the bits of
min(D, seq_len), row_bits = the bits of n - 1, each at least 1; one sort while their sum is at most 32."""
import os
import subprocess

import numpy as np
import pytest

from neighbours_cases import brute_neighbours, middle_pair, no_pair, planted_ends, planted_store, same, short_store, tie_family
from self_join_cases import brute_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key_rule(n, D, L):
    """engine.h: neighbour_key_rule, in Python"""
    bound, last = min(D, L), max(n - 1, 0)
    return max(1, bound.bit_length()), max(1, last.bit_length()), 1 if max(1, bound.bit_length()) + max(1, last.bit_length()) <= 32 else 2


def model(n, pairs, D, L, k=None, two_sorts=False, seed=0):
    rng = np.random.default_rng(seed)
    a, b, d = (pairs[f].astype(np.uint64) for f in ("query", "subject", "dist"))
    flip = rng.random(len(a)) < 0.5  # whichever row held the smaller position
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    arrival = rng.permutation(len(a))
    a, b, d = a[arrival], b[arrival], d[arrival]
    dist_bits, row_bits, sorts = key_rule(n, D, L)
    row = np.stack([a, b], axis=1).reshape(-1)  # (a; d; b) and (b; d; a), side by side as mirror_pack_kernel writes them
    nb = np.stack([b, a], axis=1).reshape(-1)
    dd = np.repeat(d, 2)
    count = len(row)
    if count == 0:
        return np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    if sorts == 1 and not two_sorts:
        shift = np.uint64(32 + dist_bits)
        assert row_bits + dist_bits <= 32 and int(dd.max()) < (1 << dist_bits) and int(row.max()) < (1 << row_bits)
        keys = np.sort((row << shift) | (dd << np.uint64(32)) | nb)
        s_row = keys >> shift
        s_dist = (keys >> np.uint64(32)) & np.uint64((1 << dist_bits) - 1)
        s_nb = keys & np.uint64(0xFFFFFFFF)
    else:
        low = (dd << np.uint64(32)) | nb
        first = np.argsort(low, kind="stable")
        low, r = low[first], row[first]
        second = np.argsort(r, kind="stable")
        low, s_row = low[second], r[second]
        s_dist, s_nb = low >> np.uint64(32), low & np.uint64(0xFFFFFFFF)
    lower = np.searchsorted(s_row, np.arange(n + 1, dtype=np.uint64), side="left").astype(np.uint64)  # one search per ROW
    assert int(lower[n]) == count
    if k is None:
        offsets, kk = lower, count
    else:
        cut = np.minimum(lower[1:] - lower[:-1], np.uint64(k))
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(cut)
        kk = k
    rank = np.arange(count, dtype=np.uint64) - lower[s_row.astype(np.int64)]
    keep = rank < np.uint64(kk)
    at = (offsets[s_row.astype(np.int64)] + rank)[keep].astype(np.int64)
    total = int(offsets[n])
    out_nb, out_d = np.full(total, 0xFFFFFFFF, dtype=np.uint32), np.full(total, 0xFFFFFFFF, dtype=np.uint32)
    out_nb[at], out_d[at] = s_nb[keep].astype(np.uint32), s_dist[keep].astype(np.uint32)
    assert len(np.unique(at)) == total  # every output slot written exactly once
    return offsets, out_nb, out_d


def gappy_store():
    """isolated rows at 0, at n - 1 and in runs between connected rows: three small families among random rows"""
    rng = np.random.default_rng(21)
    codes = rng.integers(0, 4, size=(90, 40)).astype(np.uint8)
    for base, members in ((7, (8, 9, 30)), (31, (32,)), (60, (61, 62, 88))):
        for j, m in enumerate(members):
            codes[m] = codes[base]
            codes[m, j] = (codes[m, j] + 1) % 4
    return np.ascontiguousarray(codes)


STORES = {
    "planted": lambda: planted_store(3, "nt", 30, 40),
    "planted_aa": lambda: planted_store(4, "aa", 24, 30),
    "ends": lambda: planted_ends(257),
    "gappy": gappy_store,
    "middle": lambda: middle_pair(200)[0],
    "none": lambda: no_pair(100),
    "ties": lambda: tie_family()[0],
    "short": lambda: short_store(60),
}


@pytest.mark.parametrize("name", list(STORES))
def test_model_equals_brute_force(name):
    codes = STORES[name]()
    n, L = codes.shape
    for D in ((4, 9) if name == "short" else (2, 3, 4)):
        pairs = brute_pairs(codes, min(D, L))
        whole = brute_neighbours(codes, D)
        if name == "none":
            assert len(pairs) == 0 and not whole[0].any()
        if name == "gappy":
            deg = np.diff(whole[0].astype(np.int64))
            assert deg[0] == 0 and deg[-1] == 0 and deg[7] > 0 and deg[88] > 0 and (deg[10:30] == 0).all() and (deg[33:60] == 0).all()
        if name == "short":
            assert (np.diff(whole[0].astype(np.int64)) == n - 1).all() and int(whole[2].max()) == 4
        for k in (None, 1, 2, 3, 39, 40, 41, 79, 1000):
            want = whole if k is None else brute_neighbours(codes, D, k)
            for two in (False, True):
                same(model(n, pairs, D, L, k, two_sorts=two, seed=k or 0), want)


def test_ties_at_the_cut_go_to_the_smaller_number():
    codes, is_copy = tie_family()
    offsets, nb, ds = brute_neighbours(codes, 1)
    copies = np.flatnonzero(is_copy)
    for i in range(80):
        mine = nb[int(offsets[i]):int(offsets[i + 1])]
        if is_copy[i]:
            assert len(mine) == 79 and mine[:39].tolist() == [c for c in copies if c != i]
        else:
            assert mine.tolist() == copies.tolist()  # its 40 neighbours at distance 1; the other variants are at 2
    for k in (1, 39, 40, 41, 79):
        cut = brute_neighbours(codes, 1, k)
        for i in range(80):
            full = nb[int(offsets[i]):int(offsets[i + 1])]
            assert cut[1][int(cut[0][i]):int(cut[0][i + 1])].tolist() == full[:k].tolist()


# (n, max_div, seq_len) -> (dist_bits, row_bits, sorts), by hand
KEY_CASES = [
    ((256, 3, 60), (2, 8, 1)),          # n = 2^k: n - 1 needs k bits
    ((257, 3, 60), (2, 9, 1)),          # ... 2^k + 1: one more
    ((512, 3, 60), (2, 9, 1)),
    ((513, 3, 60), (2, 10, 1)),
    ((513, 4, 60), (3, 10, 1)),         # the distance field widens from D = 3 to 4
    ((513, 7, 60), (3, 10, 1)),
    ((513, 8, 60), (4, 10, 1)),         # ... and from 7 to 8
    ((513, 0, 60), (1, 10, 1)),         # never narrower than one bit
    ((513, 100, 60), (6, 10, 1)),       # D >= seq_len: seq_len's width
    ((513, 60, 60), (6, 10, 1)),
    ((300, 9, 4), (3, 9, 1)),           # seq_len 4: distances 0..4 need 3 bits
    ((300, 4, 4), (3, 9, 1)),
    ((300, 63, 64), (6, 9, 1)),
    ((300, 64, 64), (7, 9, 1)),
    ((0, 3, 60), (2, 1, 1)),
    ((1, 3, 60), (2, 1, 1)),
    ((2, 3, 60), (2, 1, 1)),
    ((3, 3, 60), (2, 2, 1)),
    ((1 << 29, 5, 60), (3, 29, 1)),     # 29 + 3 = 32: still one key
    (((1 << 29) + 1, 5, 60), (3, 30, 2)),   # the first n that takes two sorts at D = 5
    ((1 << 30, 3, 60), (2, 30, 1)),
    (((1 << 30) + 1, 3, 60), (2, 31, 2)),   # ... and at D = 3
    ((1 << 26, 60, 60), (6, 26, 1)),
    (((1 << 26) + 1, 60, 60), (6, 27, 2)),
    (((1 << 26) + 1, 31, 60), (5, 27, 1)),  # the first D that takes two sorts at this n is 32
    (((1 << 26) + 1, 32, 60), (6, 27, 2)),
    ((0xFFFFFFF0, 0, 60), (1, 32, 2)),      # the largest store
]


def test_key_rule_table(tmp_path):
    for args, want in KEY_CASES:
        assert key_rule(*args) == want, args  # the model's rule is the table's
    src = tmp_path / "rule.cpp"
    rows = ", ".join("{%s}" % ", ".join("%dull" % v for v in args) for args, _ in KEY_CASES)
    src.write_text(
        '#include <cstdio>\n#include "%s"\n'
        "int main() {\n"
        "    const unsigned long long cases[][3] = {%s};\n"
        "    for (const auto &c : cases) {\n"
        "        const smafa::NeighbourKey r = smafa::neighbour_key_rule(c[0], (uint32_t)c[1], (uint32_t)c[2]);\n"
        '        printf("%%u %%u %%u\\n", r.dist_bits, r.row_bits, r.sorts);\n'
        "    }\n"
        "}\n" % (os.path.join(ROOT, "smafa_amd", "csrc", "engine.h"), rows))
    exe = str(tmp_path / "rule")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-o", exe, str(src)], check=True, capture_output=True, text=True)
    got = [tuple(int(v) for v in ln.split()) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(got) == len(KEY_CASES)
    for (args, want), have in zip(KEY_CASES, got):
        assert have == want, (args, want, have)

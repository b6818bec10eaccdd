"""The cluster driver's sequential pass and its two small rules (host/cluster_batch.h), from the header compiled for the host.

The header is compiled into a stand-alone program under AddressSanitizer and UBSan.  This file plays cluster_run's loop
(host/cluster.cpp) around it with the oracle standing in for the device: exact duplicates leave first, then per batch the scan
against the centroids known before the batch is reduced to every record's first row, the scan against the batch's candidates is
passed whole, and the program resolves the batch.  The record -> centroid assignment must be the oracle's sequential one.

Four situations decide whether the pass is right, and the synthetic cases are chosen (seeds tried on the CPU) so that each occurs:
a record whose nearest centroid lies at exactly D (it joins) or at D + 1 (it does not); a record as near to an old centroid as to
a new one of its batch (the old one wins); a record equally near to two new ones (the earlier wins); a record within D of an
earlier candidate that did not become a centroid, nearer than any centroid (it must not join it)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from smafa_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "smafa_amd", "csrc", "host", "cluster_batch.h")
NONE = 0xFFFFFFFF

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "%s"
static std::vector<uint32_t> numbers(size_t n) {
    std::vector<uint32_t> v(n);
    for (auto &x : v) {
        unsigned long long t = 0;
        if (scanf("%%llu", &t) != 1) exit(3);
        x = (uint32_t)t;
    }
    return v;
}
static void print(const std::vector<uint32_t> &v) {
    for (uint32_t x : v) printf("%%u ", x);
    printf("\n");
}
int main() {
    char what = 0;
    while (scanf(" %%c", &what) == 1) {
        if (what == 'R') {  // nb max_divergence next_centroid n_cand n_hits, then old_d, old_c, cand_pos, the rows
            const std::vector<uint32_t> h = numbers(5);
            const std::vector<uint32_t> old_d = numbers(h[0]), old_c = numbers(h[0]), cand_pos = numbers(h[3]), flat = numbers(3 * (size_t)h[4]);
            std::vector<smafa_hit> rows(h[4]);
            for (size_t t = 0; t < rows.size(); t++) rows[t] = {flat[3 * t], flat[3 * t + 1], flat[3 * t + 2]};
            std::vector<uint32_t> centroid, became;
            smafa::resolve_batch(h[0], old_d.data(), old_c.data(), cand_pos, rows.data(), rows.size(), h[1], h[2], centroid, became);
            print(centroid);
            print(became);
        } else if (what == 'S') {  // nb rank world
            const std::vector<uint32_t> a = numbers(3);
            printf("%%zu\n", smafa::slice_start(a[0], a[1], a[2]));
        } else if (what == 'B') {  // B batch_cap nb n_cand n_rows
            const std::vector<uint32_t> a = numbers(5);
            printf("%%zu\n", smafa::next_batch_size(a[0], a[1], a[2], a[3], a[4]));
        } else {
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}
"""


class Program:
    """the compiled header behind a pipe: one request, one answer"""

    def __init__(self, exe):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def ask(self, request, lines):
        self.p.stdin.write(request + "\n")
        self.p.stdin.flush()
        out = [self.p.stdout.readline() for _ in range(lines)]
        assert all(ln.endswith("\n") for ln in out), "the program ended early: " + self.close()[1]
        return [[int(x) for x in ln.split()] for ln in out]

    def close(self):
        self.p.stdin.close()
        err = self.p.stderr.read()
        return self.p.wait(), err


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cluster_batch")
    src = tmp / "model.cpp"
    src.write_text(PROGRAM % HEADER)
    exe = str(tmp / "model")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", exe, str(src)], check=True, capture_output=True, text=True)
    prog = Program(exe)
    yield prog
    status, err = prog.close()
    assert status == 0 and "Sanitizer" not in err and "runtime error" not in err, (status, err)


def distance_matrix(codes):
    return np.stack([oracle.distances_codes(codes, row) for row in codes]).astype(np.int64)


def play(program, codes, D, batch, seen):
    """cluster_run's loop over `codes` in batches of `batch` records -> centroid ordinal per record; `seen` counts the situations"""
    first = {}
    uniq = [i for i, row in enumerate(codes) if first.setdefault(row.tobytes(), i) == i]  # as first_occurrences does
    dist = distance_matrix(codes)
    centroid_of = np.full(len(codes), NONE, dtype=np.uint32)
    centroid_rec = []
    for pos in range(0, len(uniq), batch):
        idx = uniq[pos:pos + batch]
        nb, rows = len(idx), codes[idx]
        old_d, old_c = [NONE] * nb, [NONE] * nb
        n_old = len(centroid_rec)
        if n_old:
            for q, c, d in oracle.scan_codes(codes[centroid_rec], rows, D)[::-1].tolist():  # backwards: the first row of each record wins
                old_d[q], old_c[q] = d, c
        cand_pos = [b for b in range(nb) if old_c[b] == NONE]
        hits = oracle.scan_codes(rows[cand_pos], rows, D).tolist() if cand_pos else []
        request = ["R %d %d %d %d %d" % (nb, D, n_old, len(cand_pos), len(hits)), *(" ".join(map(str, v)) for v in (old_d, old_c, cand_pos)),
                   " ".join("%d %d %d" % row for row in hits)]
        centroid, became = program.ask("\n".join(request), 2)
        assert len(centroid) == nb and became == sorted(set(became)) and set(became) <= set(cand_pos)
        centroid_of[idx] = centroid
        centroid_rec += [idx[b] for b in became]
        # the situations, from all distances (not from what the program was given)
        for b, i in enumerate(idx):
            new = [idx[j] for j in became if j < b]
            d_old = dist[i, centroid_rec[:n_old]].min() if n_old else 1 << 30
            d_new = dist[i, new].min() if new else 1 << 30
            d_min = min(d_old, d_new)
            seen["exactly D"] += d_min == D
            seen["D + 1"] += d_min == D + 1
            seen["old ties new"] += d_old == d_new <= D
            seen["new ties new"] += d_new <= D and d_new < d_old and (dist[i, new] == d_new).sum() > 1
            shunned = [idx[j] for j in cand_pos if j < b and j not in became]
            seen["a nearer candidate that is no centroid"] += bool(shunned) and dist[i, shunned].min() <= min(D, d_min - 1)
    return centroid_of


def situations():
    return {"exactly D": 0, "D + 1": 0, "old ties new": 0, "new ties new": 0, "a nearer candidate that is no centroid": 0}


# Eight records of length 8 and a duplicate at D = 2, two batches of four; the centroid of each, worked out by hand.
HAND = [
    (b"AAAAAAAA", 0),     # the first record: centroid 0
    (b"AAAAAACC", 0),     # 2 = D from centroid 0: joins it
    (b"AAAAACCC", 1),     # 3 = D + 1 from centroid 0; 1 from the record above, which is no centroid: centroid 1
    (b"AAAAAACG", 0),     # 2 from centroid 0 and 2 from centroid 1, both new in this batch: the earlier
    (b"TTTTAAAA", 2),     # second batch.  4 from centroid 0: centroid 2
    (b"AATTAAAA", 0),     # 2 from the old centroid 0 and 2 from centroid 2, new in this batch: the old one
    (b"ATTTAAAA", 2),     # 3 from centroid 0, 1 from centroid 2: joins it
    (b"ACTTAAAG", 3),     # 2 from the record above, which is no centroid; 3 from centroid 2, 4 from centroid 0: centroid 3
    (b"AAAAAACC", NONE),  # a duplicate of the second record: skipped
]


def test_hand_made_batches(program):
    codes = oracle.codes_from_ascii(np.frombuffer(b"".join(row for row, _ in HAND), dtype=np.uint8).reshape(len(HAND), 8), oracle.ALPHABET_NT)
    want = np.array([c for _, c in HAND], dtype=np.uint32)
    assert (oracle.cluster_codes(codes, 2, oracle.ALPHABET_NT) == want).all()
    seen = situations()
    assert (play(program, codes, 2, 4, seen) == want).all()
    assert seen == {"exactly D": 3, "D + 1": 2, "old ties new": 1, "new ties new": 1, "a nearer candidate that is no centroid": 3}, seen
    for batch in (1, 3, 9):
        assert (play(program, codes, 2, batch, situations()) == want).all(), batch


AA_SEED, NT_SEED = 4, 4


def test_synthetic_batches_equal_the_sequential_oracle(program):
    seen = situations()
    aa = synth.cluster_records(40, 12, 60, alphabet=1, seed=AA_SEED, max_subs=4)
    nt = synth.cluster_records(24, 10, 60, alphabet=0, seed=NT_SEED, max_subs=4)
    for codes, alphabet in ((aa, oracle.ALPHABET_AA), (nt, oracle.ALPHABET_NT)):
        for D in (5, 2):
            want = oracle.cluster_codes(codes, D, alphabet)
            for batch in (1, 7, 64, len(codes)):
                got = play(program, codes, D, batch, seen)
                assert (got == want).all(), (alphabet, D, batch, np.nonzero(got != want)[0][:8])
    assert all(count > 0 for count in seen.values()), seen


def test_slice_and_batch_size_rules(program):
    # (nb, rank, world) -> where the rank's slice starts; rank = world: where the last one ends
    slices = [((10, 0, 3), 0), ((10, 1, 3), 3), ((10, 2, 3), 6), ((10, 3, 3), 10), ((1, 0, 2), 0), ((1, 1, 2), 0), ((1, 2, 2), 1),
              ((0, 1, 2), 0), ((7, 0, 1), 0), ((7, 1, 1), 7), ((65536, 1, 3), 21845), ((65536, 2, 3), 43690), ((65536, 63, 64), 64512)]
    for args, want in slices:
        assert program.ask("S %d %d %d" % args, 1) == [[want]], args
    M = 1 << 20
    # (B, batch_cap, nb, candidates, candidate rows) -> the next B; the volume is nb - candidates + rows
    sizes = [
        ((1024, 65536, 1024, 0, 0), 2048),                 # a cheap batch: twice the size
        ((32768, 65536, 32768, 32768, 0), 65536),          # ... up to the cap
        ((65536, 65536, 65536, 0, 0), 65536),              # ... and not past it
        ((1024, 256, 10, 0, 0), 1024),                     # (a cap below B does not shrink it)
        ((1024, 65536, 1024, 1024, 4 * M - 1), 2048),      # just under 4M rows
        ((1024, 65536, 1024, 1024, 4 * M), 1024),          # 4M: as it is
        ((1024, 65536, 1024, 24, 4 * M - 1000), 1024),     # the records with an old centroid count too
        ((1024, 65536, 1024, 1024, 16 * M), 1024),         # 16M: as it is
        ((1024, 65536, 1024, 1024, 16 * M + 1), 512),      # above: half the size
        ((512, 65536, 512, 512, 17 * M), 256),             # ... down to 256
        ((256, 65536, 256, 256, 17 * M), 256),             # ... and not below
        ((65536, 65536, 65536, 65536, 17 * M), 32768),
    ]
    for args, want in sizes:
        assert program.ask("B %d %d %d %d %d" % args, 1) == [[want]], args

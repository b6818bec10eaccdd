"""Expected answers of the density tests (tests/test_density_model.py, tests/test_gpu_density.py, tests/density_worker.py).

Nothing here comes from the code under test: the pairs are self_join_cases.brute_pairs — brute force on the code bytes —
the degrees a bincount over both of their columns, the core labels components_cases.labels_from_pairs over the core-core
pairs, and a border row's label that of its smallest-numbered core neighbour."""
import numpy as np

from components_cases import labels_from_pairs
from self_join_cases import brute_pairs

NONE = 0xFFFFFFFF


def density_from_pairs(n, pairs, min_pts):
    """pairs (HIT_DTYPE, each unordered pair once) -> (labels uint32[n], degrees uint32[n], counts)"""
    min_pts = max(int(min_pts), 1)
    q, s = pairs["query"].astype(np.int64), pairs["subject"].astype(np.int64)
    degrees = np.bincount(q, minlength=n) + np.bincount(s, minlength=n)
    core = degrees + 1 >= min_pts
    both = core[q] & core[s]
    roots = labels_from_pairs(n, pairs[both]).astype(np.int64)  # (a non-core row is in no core-core pair: a set of its own)
    attach = np.full(n, NONE, dtype=np.int64)  # the smallest core NUMBER within the bound of a non-core row
    left, right = core[q] & ~core[s], ~core[q] & core[s]
    np.minimum.at(attach, s[left], q[left])
    np.minimum.at(attach, q[right], s[right])
    labels = np.full(n, NONE, dtype=np.int64)
    labels[core] = roots[core]
    border = ~core & (attach != NONE)
    labels[border] = roots[attach[border]]
    counts = {"clusters": int((core & (roots == np.arange(n))).sum()), "core": int(core.sum()),
              "noise": int((labels == NONE).sum())}
    return labels.astype(np.uint32), degrees.astype(np.uint32), counts


def brute_density(codes, D, min_pts):
    """-> (labels, degrees, counts) of a store at bound D and min_pts"""
    return density_from_pairs(len(codes), brute_pairs(codes, D), min_pts)


def kinds(labels, degrees, min_pts):
    """-> boolean masks (core, border, noise)"""
    core = degrees.astype(np.int64) + 1 >= max(int(min_pts), 1)
    noise = labels == NONE
    return core, ~core & ~noise, noise


def bridged_store(seed, copies=32, steps=12, L=60):
    """Two families of `copies` exact copies each, of two rows `steps` columns apart, bridged by a chain of steps - 1 single
    rows that walks from the one to the other, one column per step (components_cases.chain_store's idea): consecutive rows
    of the walk differ in exactly one column, rows two steps apart in two.  Shuffled.
    -> (codes, role of every row): role 0 / 1 = a copy of family 0 / 1, role 2 + k = row k of the chain, k = 0 .. steps - 2.

    At D = 1 single linkage chains the two families into ONE component.  At min_pts = 4 every chain row but the two
    outermost has exactly 2 neighbours and is not core, so the answer has exactly 2 clusters.  (The two outermost chain rows
    are within 1 of a whole family — `copies` + 1 neighbours — and are core members of its cluster: a row within the bound of
    32 copies cannot be anything else.  The border rows are the next two, whose one core neighbour is an outermost row, and
    the steps - 5 rows between them are noise.)  These facts are asserted here on the brute-force answer, so that a change
    of the generator cannot hollow the tests out."""
    assert copies >= 30 and steps >= 8
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, size=L).astype(np.uint8)
    cols = rng.choice(L, size=steps, replace=False)
    rows, role = [a] * copies, [0] * copies
    row = a.copy()
    for k, c in enumerate(cols):
        row = row.copy()
        row[c] = (row[c] + 1 + rng.integers(0, 3)) % 4
        if k < steps - 1:
            rows.append(row)
            role.append(2 + k)
    rows += [row] * copies  # the far end of the walk is the second family
    role += [1] * copies
    perm = rng.permutation(len(rows))
    codes = np.ascontiguousarray(np.array(rows, dtype=np.uint8)[perm])
    role = np.array(role)[perm]
    # the facts, from brute force
    n, chain = len(codes), steps - 1
    pairs = brute_pairs(codes, 1)
    assert len(set(labels_from_pairs(n, pairs).tolist())) == 1  # one component
    labels, degrees, counts = density_from_pairs(n, pairs, 4)
    core, border, noise = kinds(labels, degrees, 4)
    where = {k: int(np.flatnonzero(role == 2 + k)[0]) for k in range(chain)}
    assert all(degrees[where[k]] == 2 and not core[where[k]] for k in range(1, chain - 1))
    assert degrees[where[0]] == copies + 1 and degrees[where[chain - 1]] == copies + 1
    assert (degrees[role < 2] == copies).all() and core[role < 2].all()
    assert counts == {"clusters": 2, "core": 2 * copies + 2, "noise": chain - 4}, counts
    assert sorted(np.flatnonzero(border).tolist()) == sorted([where[1], where[chain - 2]])
    assert sorted(np.flatnonzero(noise).tolist()) == sorted(where[k] for k in range(2, chain - 2))
    assert labels[where[1]] == labels[where[0]] != labels[where[chain - 2]] == labels[where[chain - 1]]
    assert len(set(labels[role == 0].tolist())) == 1 and len(set(labels[role == 1].tolist())) == 1
    return codes, role

"""What the stable-cluster tests hold an answer to (tests/test_gpu_stable.py, tests/stable_worker.py, tests/test_stable_model.py).

Nothing here comes from the code under test.  The levels are reach_cases.expected_reach — cores and the partition at every weight
0 .. D by brute force on the code bytes — and the selection is the definition of include/smafa_amd.h written down as it reads,
in plain loops over levels and clusters: sizes of the rows that are in, big components, kids, chains, stability, excess of mass."""
import hashlib

import numpy as np

from reach_cases import NONE, expected_reach

_SELECTED = {}


def cluster_tree(cores, labels, S):
    """cores uint32[n], labels (D + 1, n) -> the clusters, children before parents: dicts with chain = [(t, r)], t_lo, t_hi, r_hi,
    stability, parent (index or None), children (indices), best, chosen"""
    levels, n = labels.shape
    S = int(S)
    assert S >= 1
    cores = np.asarray(cores).astype(np.int64)  # (NONE is above every level)
    clusters, of_component, size_below = [], {}, {}
    for t in range(levels):
        inside = cores <= t
        roots, counts = np.unique(labels[t][inside], return_counts=True)
        size = {int(r): int(c) for r, c in zip(roots, counts)}
        kids = {}
        for r in sorted(size_below):  # the big components of the level below
            if size_below[r] >= S:
                kids.setdefault(int(labels[t][r]), []).append(r)
        for r in sorted(size):
            if size[r] < S:
                continue
            mine = kids.get(r, [])
            if len(mine) == 1:
                c = of_component[(t - 1, mine[0])]
            else:
                c = len(clusters)
                clusters.append({"chain": [], "t_lo": t, "stability": 0, "parent": None, "children": []})
                for kid in mine:
                    child = of_component[(t - 1, kid)]
                    clusters[child]["parent"] = c
                    clusters[c]["children"].append(child)
            of_component[(t, r)] = c
            clusters[c]["chain"].append((t, r))
            clusters[c]["t_hi"], clusters[c]["r_hi"] = t, r
            clusters[c]["stability"] += size[r]
        assert all(k in size and size[k] >= S for k in kids)  # a big child's component is big
        size_below = size
    for c in clusters:  # (a child has a smaller index than its parent: it was started at a lower level)
        below = sum(clusters[k]["best"] for k in c["children"])
        c["best"] = max(c["stability"], below)
        c["wins"] = c["stability"] >= below
    for c in reversed(clusters):
        up = clusters[c["parent"]] if c["parent"] is not None else None
        c["closed"] = bool(up and (up["chosen"] or up["closed"]))
        c["chosen"] = c["wins"] and not c["closed"]
    return clusters


def select_stable(cores, labels, S):
    """-> (labels uint32[n], joined uint32[n], n_clusters) of the definition"""
    levels, n = labels.shape
    cores64 = np.asarray(cores).astype(np.int64)
    out = np.full(n, NONE, dtype=np.uint32)
    joined = np.full(n, NONE, dtype=np.uint32)
    count = 0
    for c in cluster_tree(cores, labels, S):
        if not c["chosen"]:
            continue
        count += 1
        for t, r in c["chain"]:
            rows = (cores64 <= t) & (labels[t] == r)
            assert (out[rows] == NONE).all() or (out[rows][out[rows] != NONE] == c["r_hi"]).all()  # at most one cluster a row
            fresh = rows & (joined == NONE)
            joined[fresh] = t
            out[rows] = c["r_hi"]
    return out, joined, count


def sizes(M, S):
    M = max(int(M), 1)
    return M, int(S) if S else M


def expected_stable(codes, D, M, S):
    """(labels, joined, n_clusters, cores) by brute force, once per store and parameters"""
    M, S = sizes(M, S)
    key = (hashlib.sha1(np.ascontiguousarray(codes).tobytes()).hexdigest(), codes.shape, int(D), M, S)
    if key not in _SELECTED:
        cores, labels, _ = expected_reach(codes, D, M)
        out, joined, count = select_stable(cores, labels, S)
        out.setflags(write=False)
        joined.setflags(write=False)
        _SELECTED[key] = (out, joined, count, cores)
    return _SELECTED[key]


def check_stable(codes, out, D, M, S):
    """out = (labels, n_clusters, joined, cores) as SubjectStore.self_stable_clusters(D, M, S, joined=True, cores=True) returns
    them: every output byte for byte, the cores against the brute cores"""
    n = len(codes)
    labels, count, joined, cores = out
    want, want_joined, want_count, want_cores = expected_stable(codes, D, M, S)
    for a in (labels, joined, cores):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (n,), (a.dtype, a.shape)
    assert cores.tobytes() == want_cores.tobytes(), "cores differ from brute force at rows %s" % np.flatnonzero(cores != want_cores)[:8]
    assert labels.tobytes() == want.tobytes(), "labels differ at rows %s: %s, expected %s" % (
        np.flatnonzero(labels != want)[:8], labels[labels != want][:8], want[labels != want][:8])
    assert joined.tobytes() == want_joined.tobytes(), "joined differs at rows %s" % np.flatnonzero(joined != want_joined)[:8]
    assert isinstance(count, int) and count == want_count, (count, want_count)
    return want_count


def traits(cores, labels, S):
    """what a fixture's expected answer contains (tests/test_stable_model.py): -> a set of words"""
    clusters = cluster_tree(cores, labels, S)
    out, joined, _ = select_stable(cores, labels, S)
    found = set()
    for c in clusters:
        if c["chosen"] and c["children"]:
            found.add("chosen non-leaf")
        if c["chosen"] and not c["children"] and c["parent"] is not None and not clusters[c["parent"]]["chosen"]:
            found.add("chosen leaf under a parent that is not")
        if c["chosen"]:
            found.add("t_hi %d" % c["t_hi"])
            mine = out == c["r_hi"]
            if (joined[mine] > c["t_lo"]).any():
                found.add("joined later")
    if (out == NONE).any():
        found.add("noise")
    return found


# ---- the stores of tests/test_gpu_stable.py that must not be trivial, as (name, maker of the codes, D, M, S): what their expected
# answers contain together is asserted on the CPU (tests/test_stable_model.py::test_gpu_fixtures_are_not_trivial)
def bridged_codes():
    from density_cases import bridged_store

    return bridged_store(5)[0]


def short_codes():
    """420 rows of 3 columns in families of ten, up to two columns from their seed: many copies, every distance 0 .. 3"""
    from self_join_cases import planted_store

    return planted_store(5, "nt", 3, 40, max_subs=2)


def planted_codes(kind):
    """1 520 rows of 60 columns in families of ten (aa: two words a plane), or 1 520 nt rows with N in 1 % of the columns"""
    from self_join_cases import planted_store

    return planted_store(77, kind[:2], 60, 150, 0.01 if kind == "ntn" else 0.0)


FIXTURES = [
    ("bridged", bridged_codes, 3, 4, 0),
    ("bridged", bridged_codes, 3, 2, 5),
    ("short", short_codes, 2, 3, 5),
    ("short", short_codes, 6, 1, 0),
    ("aa", lambda: planted_codes("aa"), 5, 2, 5),
    ("aa", lambda: planted_codes("aa"), 5, 4, 0),
    ("ntn", lambda: planted_codes("ntn"), 5, 2, 0),
    ("ntn", lambda: planted_codes("ntn"), 5, 1, 1),
]

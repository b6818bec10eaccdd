"""The kernel choice of a scan launch (smafa_amd/csrc/scan_plan.h: plan_scan, scan_kernel_name), from the header compiled for
the host: g++ alone, no HIP — that the header compiles this way is part of the test.

(a) Every census case that is ONE fixed-bound launch (tests/kernel_census_table.py: D given, k == 0, no index) must get the
    census's own name from the plan, its inputs derived from the case.  The GPU census then runs the same cases on a device.
(b) A hand-worked table for what the census cannot reach: the seed and per-query forms, the rules between the kernel families,
    the zone level's pass-share thresholds, and the two bound predicates on both sides of their bounds.  The expected values
    are worked from the rules as the comments of scan_plan.h state them:
      * level 1 prunes while P(Binomial(cols, 1/2) <= bound) <= 2e-3, cols = min(32, L): 32 columns 4 514 873 / 2^32 = 1.05e-3
        at bound 7, 3.5e-3 at 8; 20 columns 1351 / 2^20 = 1.3e-3 at 3, 5.9e-3 at 4; 12 columns 1 / 4096 at 0, 13 / 4096 at 1;
      * level 2 of a two-word store of at least 56 columns rejects while 2 x bound <= (3 s + 2 (32 - s)) / 4 + 1, s = L - 32
        (60 columns: 23, so up to 12), and up to 14 by the per-word sums;
      * the zone level pays below a pass share of 0.6 (0.4 for P x W >= 20 up to four words), below SMAFA_ZONE_LOOSE = 0.3 where
        level 1 does not prune; a store whose tiles all share b bits passes P(Binomial(b, 1/2) <= bound): bound 5, 12 bits
        1586 / 4096 = 0.39, 10 bits 638 / 1024 = 0.62.
(c) For every row of (a) and (b) the plan's tiles per wave and waves per workgroup — what the grid is sized by — must be what
    the NAMED kernel is compiled with (zone_tiles, kFewTiles, kWideTiles, kGenericTiles; kZoneWgWaves for scan_zone_kernel).
    For the zone, few-query, wide and generic kernels that is an independent check: T is no part of their names.  scan_kernel
    and scan_lazy_kernel carry T in their names, which are printed from the plan, so for those two (c) only checks the waves;
    their T is held by the names expected in (a) and (b) and by launch_scan's guards (engine.hip), which refuse a plan whose T
    the named instantiation does not have.

One rule of the plan cannot be shown by any row: scan_lazy_kernel's sumfold is decided without use_filter, but the kernel is
only ever chosen with the filter on, so no input tells the two readings apart.  The rows at bounds 12..15 pin what can be seen
of it: sumfold exactly at 13 and 14 with the filter on, and scan_kernel's fold 0 with it off."""
import os
import re
import subprocess

import pytest

from kernel_census_table import CENSUS, PSPQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "smafa_amd", "csrc", "scan_plan.h")

KNOBS = dict(lazy=1, filter=1, wide_one=1, wide_from=5, tiles=0, zone=1, loose=0.3, direct=1, lazy_fold=1, fold3=1)
SWITCH_KNOBS = {"default": {}, "tiles4": dict(tiles=4), "tiles2": dict(tiles=2), "wide_one_off": dict(wide_one=0),
                "wide_from3": dict(wide_from=3), "zone_staged": dict(direct=0)}


def row(kind, L, thr0, nq=129, seed=0, rows=1, per_query=0, share=1.0, bits=-1, **knobs):
    """one launch: share — the pass share as a value; bits >= 0 — as the histogram of a store whose tiles all share `bits` bits"""
    assert not set(knobs) - set(KNOBS), knobs
    P, PQ = PSPQ[kind]
    return dict(KNOBS, P=P, PQ=PQ, W=(L + 31) // 32, L=L, thr0=thr0, nq=nq, seed=seed, rows=rows, per_query=per_query,
                share=share, bits=bits, **knobs)


def census_rows():
    out = []
    for name, cases in CENSUS.items():
        for c in cases:
            if c["D"] is None or c["k"] != 0 or c["index"]:
                continue
            # (the zone level off must not look at the share, so it gets one that would pay; forced, one that would not)
            r = row(c["kind"], c["L"], min(c["D"], c["L"]), nq=c["nq"], share=0.0 if c["zone"] == 0 else 1.0,
                    filter=int(c["prefilter"]), zone=c["zone"], **SWITCH_KNOBS[c["switches"]])
            out.append((r, name + (" (%s)" % c["marker"] if c["marker"] else "")))
    return out


SK, LK, ZK, WK = "smafa::scan_kernel<%s>", "smafa::scan_lazy_kernel<%s>", "smafa::scan_zone_kernel<%s>", "smafa::scan_wide_kernel<%s>"
HAND = [
    # a seed launch (no row list, k = 1) never takes the zone level, forced or not, and runs the `true` instantiations
    (row("aa", 60, 60, seed=1, rows=0, per_query=1, zone=2), SK % "5, 5, 2, 1, true, 0"),
    (row("aa", 60, 5, seed=1, rows=0, per_query=1, zone=2), LK % "5, 5, 2, 4, true, false"),
    (row("aa", 31, 5, seed=1, rows=0, per_query=1, zone=2), WK % "5, 5, true, 1, 0"),
    (row("aa", 150, 5, seed=1, rows=0, per_query=1, zone=2), WK % "5, 5, true, 3, 0"),  # ... nor scan_wide_kernel's own
    # per-query bounds with the zone level forced: the staged, per-query form
    (row("aa", 60, 60, per_query=1, zone=2), ZK % "5, 5, 2, false, false"),
    # the zone kernel only up to four words per plane: five words have it inside scan_wide_kernel, or not at all
    (row("aa", 150, 5, zone=2), WK % "5, 5, false, 3, 0" + " (zone level on)"),
    (row("aa", 150, 20, zone=2), "smafa::scan_generic_kernel"),
    # zone wins over wide for one-word stores
    (row("aa", 31, 5, zone=2), ZK % "5, 5, 1, true, true"),
    # the few-query form up to 64 queries (kFewTiles, four waves), the zone kernel from 65
    (row("aa", 60, 5, nq=64, zone=2), "smafa::scan_zone_few_kernel<5, 5, 2>"),
    (row("aa", 60, 5, nq=1, zone=2), "smafa::scan_zone_few_kernel<5, 5, 2>"),
    (row("aa", 60, 5, nq=65, zone=2), ZK % "5, 5, 2, true, true"),
    # direct requires a fixed bound, zone_direct and a row list
    (row("aa", 60, 5, zone=2, rows=0), ZK % "5, 5, 2, true, false"),
    (row("aa", 60, 5, zone=2, direct=0), ZK % "5, 5, 2, true, false"),
    (row("aa", 60, 5, zone=2, per_query=1), ZK % "5, 5, 2, false, false"),
    # the lazy kernel's sumfold at 13..17 (fold_rejects sends it 13 and 14); scan_kernel's fold looks at use_filter (filter off:
    # fold 0 at the same bounds, one tile per wave)
    (row("aa", 60, 12), LK % "5, 5, 2, 4, false, false"),
    (row("aa", 60, 13), LK % "5, 5, 2, 4, false, true"),
    (row("aa", 60, 14), LK % "5, 5, 2, 4, false, true"),
    (row("aa", 60, 15), SK % "5, 5, 2, 2, false, 1"),
    (row("aa", 60, 13, lazy_fold=0), SK % "5, 5, 2, 2, false, 1"),
    (row("aa", 60, 13, filter=0), SK % "5, 5, 2, 1, false, 0"),
    (row("aa", 60, 15, filter=0), SK % "5, 5, 2, 1, false, 0"),
    # fold 3 (all planes but the last, above 32) needs four planes; three planes get fold 2 there; SMAFA_FOLD3=0: neither
    (row("aa", 60, 40), SK % "5, 5, 2, 1, false, 3"),
    (row("nt2", 60, 40), SK % "2, 3, 2, 1, false, 0"),
    (row("nt3", 60, 40), SK % "3, 3, 2, 1, false, 2"),
    (row("aa", 60, 40, fold3=0), SK % "5, 5, 2, 1, false, 0"),
    (row("nt3", 60, 40, fold3=0), SK % "3, 3, 2, 1, false, 0"),
    (row("nt2", 60, 24), SK % "2, 3, 2, 1, false, 0"),  # (fold 2 at 18..32 from three planes on)
    # SMAFA_TILES=4: two tiles per wave on stores of three and more planes, four on two
    (row("aa", 45, 10, tiles=4), SK % "5, 5, 2, 2, false, 0"),
    (row("nt3", 45, 10, tiles=4), SK % "3, 3, 2, 2, false, 0"),
    (row("nt2", 45, 10, tiles=4), SK % "2, 3, 2, 4, false, 0"),
    # more than two words without the lazy kernel: one tile per wave whatever SMAFA_TILES says
    (row("aa", 90, 10), SK % "5, 5, 3, 1, false, 0"),
    (row("aa", 90, 10, tiles=2), SK % "5, 5, 3, 1, false, 0"),
    (row("nt2", 120, 10, tiles=4), SK % "2, 3, 4, 1, false, 0"),
    # one tile per wave where the prefilter is off or the bound is above 16, else two
    (row("aa", 45, 16), SK % "5, 5, 2, 2, false, 1"),
    (row("aa", 45, 17), SK % "5, 5, 2, 1, false, 1"),
    (row("aa", 45, 5, filter=0), SK % "5, 5, 2, 1, false, 0"),
    (row("aa", 31, 10), SK % "5, 5, 1, 2, false, 0"),
    (row("aa", 31, 17), SK % "5, 5, 1, 1, false, 0"),
    # a wide shape whose record does not fit scan_wide_kernel's LDS stage (more than 768 vectors: 5 x 615 + 1 words) goes to
    # scan_generic_kernel; 5 x 614 + 1 = 3071 words are 768 vectors and fit
    (row("aa", 614 * 32, 5), WK % "5, 5, false, 3, 0"),
    (row("aa", 615 * 32, 5), "smafa::scan_generic_kernel"),
    # the filter-plane-resident kernels off: no zone level either, forced or not
    (row("aa", 60, 5, lazy=0, zone=2), SK % "5, 5, 2, 2, false, 0"),
    # zone level 1: below a pass share of 0.6 where level 1 prunes ...
    (row("aa", 60, 5, share=0.59), ZK % "5, 5, 2, true, true"),
    (row("aa", 60, 5, share=0.61), LK % "5, 5, 2, 4, false, false"),
    (row("aa", 90, 5, share=0.59), ZK % "5, 5, 3, true, true"),
    # ... 0.4 for five planes of four words (P x W = 20) ...
    (row("aa", 120, 5, share=0.39), ZK % "5, 5, 4, true, true"),
    (row("aa", 120, 5, share=0.41), LK % "5, 5, 4, 2, false, false"),
    (row("nt3", 120, 5, share=0.59), ZK % "3, 3, 4, true, true"),
    # ... but 0.6 for scan_wide_kernel's own zone level, whatever P x W
    (row("aa", 150, 5, share=0.59), WK % "5, 5, false, 3, 0" + " (zone level on)"),
    (row("aa", 150, 5, share=0.61), WK % "5, 5, false, 3, 0"),
    # ... and SMAFA_ZONE_LOOSE = 0.3 at bounds level 1 does not prune at (10 of 32 columns)
    (row("aa", 60, 10, share=0.29), ZK % "5, 5, 2, true, true"),
    (row("aa", 60, 10, share=0.31), LK % "5, 5, 2, 4, false, false"),
    (row("aa", 45, 10, share=0.29), ZK % "5, 5, 2, true, true"),
    (row("aa", 45, 10, share=0.31), SK % "5, 5, 2, 2, false, 0"),
    # the share from the histogram: every tile shares 12 bits (0.39 at bound 5), or 10 (0.62)
    (row("aa", 60, 5, bits=12), ZK % "5, 5, 2, true, true"),
    (row("aa", 60, 5, bits=10), LK % "5, 5, 2, 4, false, false"),
    # zone level 0 and 2 never look at the share
    (row("aa", 60, 5, share=0.0, zone=0), LK % "5, 5, 2, 4, false, false"),
    (row("aa", 60, 5, share=1.0, zone=2), ZK % "5, 5, 2, true, true"),
]

# (L, bound) -> prefilter_prunes and fold_rejects of a five-plane store with the default switches
PRUNES = [((32, 7), 1), ((32, 8), 0), ((20, 3), 1), ((20, 4), 0), ((12, 0), 1), ((12, 1), 0), ((60, 7), 1), ((60, 8), 0)]
FOLDS = [((60, 12), 1), ((60, 14), 1), ((60, 15), 0), ((55, 12), 0), ((55, 5), 0), ((56, 14), 1), ((90, 12), 0), ((31, 5), 0)]

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "%(header)s"
using namespace smafa;
struct Row { unsigned P, PQ, W, L, thr0, nq; int seed, rows, per_query; double share; int bits;
             int lazy, filter, wide_one; unsigned wide_from, tiles; int zone; double loose; int direct, lazy_fold, fold3; };
int main() {
    const Row rows[] = {%(rows)s};
    for (const Row &r : rows) {
        ScanKnobs k;
        k.lazy = r.lazy, k.use_filter = r.filter, k.wide_one = r.wide_one, k.wide_from = r.wide_from, k.tiles_override = r.tiles;
        k.zone = r.zone, k.zone_loose = r.loose, k.zone_direct = r.direct, k.lazy_fold = r.lazy_fold, k.fold3 = r.fold3;
        uint64_t hist[65] = {0};
        if (r.bits >= 0) hist[r.bits] = 1000;
        const ScanShape s{r.P, r.PQ, r.W, r.L};
        const ScanLaunch l{r.thr0, r.nq, r.seed != 0, r.rows != 0, r.per_query != 0, {r.bits >= 0 ? hist : nullptr, r.share}};
        const ScanPlan p = plan_scan(s, k, l);
        printf("plan\t%%s%%s\t%%u\t%%u\n", scan_kernel_name(p, s).c_str(), p.zone_on ? " (zone level on)" : "", p.T, p.wg_waves);
    }
    const unsigned bounds[][2] = {%(bounds)s};
    for (const auto &b : bounds) {
        const ScanShape s{5, 5, (b[0] + 31) / 32, b[0]};
        printf("bound\t%%d\t%%d\n", (int)prefilter_prunes(s, ScanKnobs{}, b[1]), (int)fold_rejects(s, ScanKnobs{}, b[1]));
    }
    for (int ps : {2, 3, 5})
        for (int w = 1; w <= 4; w++)
            for (int d = 0; d < 2; d++) printf("geometry\tzone %%d %%d %%d\t%%d\n", ps, w, d, zone_tiles(ps, w, d != 0));
    printf("geometry\tfew\t%%d\ngeometry\twide\t%%d\ngeometry\tgeneric\t%%d\n", kFewTiles, kWideTiles, kGenericTiles);
    printf("geometry\twg\t%%d\ngeometry\tzone_wg\t%%d\n", kWgWaves, kZoneWgWaves);
}
"""
FIELDS = ("P", "PQ", "W", "L", "thr0", "nq", "seed", "rows", "per_query", "share", "bits", "lazy", "filter", "wide_one", "wide_from",
          "tiles", "zone", "loose", "direct", "lazy_fold", "fold3")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """the header's answers: [(name, T, waves)] for census_rows() + HAND, [(prunes, fold_rejects)] for PRUNES + FOLDS, geometry"""
    tmp = tmp_path_factory.mktemp("scan_plan")
    rows = [r for r, _ in census_rows() + HAND]
    src = tmp / "plan.cpp"
    src.write_text(PROGRAM % dict(header=HEADER, rows=", ".join("{%s}" % ", ".join(repr(r[f]) for f in FIELDS) for r in rows),
                                  bounds=", ".join("{%d, %d}" % lb for lb, _ in PRUNES + FOLDS)))
    exe = str(tmp / "plan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-o", exe, str(src)], check=True,
                   capture_output=True, text=True)
    lines = [ln.split("\t") for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    plans = [(f[1], int(f[2]), int(f[3])) for f in lines if f[0] == "plan"]
    bounds = [(int(f[1]), int(f[2])) for f in lines if f[0] == "bound"]
    geometry = {f[1]: int(f[2]) for f in lines if f[0] == "geometry"}
    assert len(plans) == len(rows) and len(bounds) == len(PRUNES) + len(FOLDS)
    return plans, bounds, geometry


def test_every_fixed_bound_census_case_gets_its_name(model):
    plans, _, _ = model
    cases = census_rows()
    # (pinned from the table as it stands: a case that drops out of the filter above fails here)
    assert len(cases) == 100 and len({name.split(" (")[0] for _, name in cases}) == 97
    for (r, want), (have, _, _) in zip(cases, plans):
        assert have == want, (r, want, have)


def test_hand_worked_table(model):
    plans, _, _ = model
    for (r, want), (have, _, _) in zip(HAND, plans[len(census_rows()):]):
        assert have == want, (r, want, have)


def test_bound_predicates_on_both_sides_of_their_bounds(model):
    _, bounds, _ = model
    for (lb, want), (prunes, _) in zip(PRUNES, bounds):
        assert prunes == want, ("prefilter_prunes", lb, want, prunes)
    for (lb, want), (_, fold) in zip(FOLDS, bounds[len(PRUNES):]):
        assert fold == want, ("fold_rejects", lb, want, fold)


def test_the_plan_sizes_the_grid_by_the_named_kernels_geometry(model):
    plans, _, g = model
    assert len(plans) == 100 + len(HAND)
    for name, T, waves in plans:
        args = [a.strip() for a in re.search(r"<(.*)>", name).group(1).split(",")] if "<" in name else []
        if name.startswith("smafa::scan_zone_kernel<"):
            want = (g["zone %s %s %d" % (args[0], args[2], args[4] == "true")], g["zone_wg"])
        elif name.startswith("smafa::scan_zone_few_kernel<"):
            want = (g["few"], g["wg"])
        elif name.startswith("smafa::scan_wide_kernel<"):
            want = (g["wide"], g["wg"])
        elif name.startswith("smafa::scan_generic_kernel"):
            want = (g["generic"], g["wg"])
        else:  # scan_kernel and scan_lazy_kernel carry T as their fourth template argument
            assert name.startswith(("smafa::scan_kernel<", "smafa::scan_lazy_kernel<")), name
            want = (int(args[3]), g["wg"])
        assert (T, waves) == want, (name, T, waves, want)

"""The k-nearest rules of smafa_amd/csrc/kth_plan.h, asked of the header itself: a small driver with its own main, compiled
with g++ alone (no HIP), that answers one question per input line.  Used by tests/test_kth_plan_model.py (CPU: every rule against
hand-worked values) and tests/test_gpu_kth_schedule.py (GPU: the launches of a call against kth_schedule).  Test helper only.

Questions (blank-separated integers unless said otherwise) and answers:
  ladder L W P n_queries                           -> the bounds
  with_index served limit b0 b1 ..                 -> index_first, then the bounds
  charge nq n vectors fixed|loose                  -> ms (%.17g)
  due debt_ms blocks n                             -> 0 | 1
  blocks aa P n L                                  -> index_blocks_wanted (at most 32)
  fixed_wants mode filter nq W thr0 L n min_rows current B failed  -> 0 | 1   (kIndexMaxWords 4, kIndexMaxBlocks 32)
  loose_pays mode filter lazy two_phase k nq limit first W n min_rows failed -> 0 | 1
  loose_wants want first current B                 -> 0 | 1
  runs k filter lazy two_phase nq                  -> ladder_runs
  probed laddered ladder_probe nq limit first index_first -> first_step_probed
  skips finished ns                                -> first_step_probe_skips
  plans_now planned open step n_steps              -> plans_later_now
  sample open                                      -> planner_sample
  later from limit b0 b1 ..                        -> any last
  step_cost bound cols                             -> %.2f
  choose cols from last n_bounds b.. ns kth..      -> mask cost (%.6f); kth -1: fewer than k rows within the last bound
  paid finished open next_bound                    -> step_paid
  count_first k count_first_k P PQ W L thr0        -> kth_count_first (default switches)
  hist_seed k L enabled                            -> kth_hist_seed (kSeedBins 256)
  sample_tiles count_first div min_tiles n_tiles k -> kth_sample_tiles
  scratch_rows count_first sample_tiles nq k cap   -> kth_scratch_rows
  hist_groups counting tiles n_chunks n_cu override -> kth_hist_groups
  schedule n_tiles k count_first sample_tiles hist_seed -> the steps, "KIND" or "KIND:begin-end" each
  capacity                                         -> kKthScheduleMax
Step kinds are spelled Z (ZeroCounts), SH (SeedHist), SS (SeedScan), MH (SampleHist), C (Count), A (CountAppend), B
(BoundsFromCounts), XS (FixedAppendScratch), XC (FixedAppendCaller), F (Filter)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "smafa_amd", "csrc", "kth_plan.h")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "%(header)s"
using namespace smafa;
static const char *kind_name(KthStep k) {
    switch (k) {
    case KthStep::ZeroCounts: return "Z";
    case KthStep::SeedHist: return "SH";
    case KthStep::SeedScan: return "SS";
    case KthStep::SampleHist: return "MH";
    case KthStep::Count: return "C";
    case KthStep::CountAppend: return "A";
    case KthStep::BoundsFromCounts: return "B";
    case KthStep::FixedAppendScratch: return "XS";
    case KthStep::FixedAppendCaller: return "XC";
    case KthStep::Filter: return "F";
    }
    return "?";
}
static void print_ladder(const LadderBounds &l) {
    for (uint32_t i = 0; i < l.n; i++) printf(" %%u", l[i]);
    printf("\n");
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        std::vector<double> v;
        std::string word;
        std::string rate;
        while (in >> word) {
            if (word == "fixed" || word == "loose") rate = word;
            else v.push_back(strtod(word.c_str(), nullptr));
        }
        auto u = [&](size_t i) { return (uint32_t)v.at(i); };
        auto u64 = [&](size_t i) { return (uint64_t)v.at(i); };
        auto b = [&](size_t i) { return v.at(i) != 0.0; };
        auto ladder_from = [&](size_t i, size_t n) {
            LadderBounds l;
            for (size_t j = 0; j < n; j++) l.push(u(i + j));
            return l;
        };
        ScanKnobs knobs;
        if (what == "ladder") {
            printf("ladder");
            print_ladder(ladder_bounds(u(0), u(1), u(2), u64(3)));
        } else if (what == "with_index") {
            LadderBounds l = ladder_from(2, v.size() - 2);
            const bool first = ladder_with_index(l, u(0), u(1));
            printf("with_index %%d", (int)first);
            print_ladder(l);
        } else if (what == "charge") {
            printf("charge %%.17g\n", index_rent_charge(u64(0), u64(1), u(2), rate == "fixed" ? kRentFixedBound : kRentLoose));
        } else if (what == "due") {
            printf("due %%d\n", (int)index_rent_due(v.at(0), u(1), u64(2)));
        } else if (what == "blocks") {
            printf("blocks %%u\n", index_blocks_wanted(b(0), u(1), u64(2), u(3), 32u));
        } else if (what == "fixed_wants") {
            knobs.use_filter = b(1);
            const IndexSite s{(int)v.at(0), u64(6), u64(7), u(3), u(5), 4u, 32u, b(8), u(9), b(10)};
            printf("fixed_wants %%d\n", (int)fixed_bound_wants_index(s, knobs, u(2), u(4)));
        } else if (what == "loose_pays") {
            knobs.use_filter = b(1), knobs.lazy = b(2);
            const IndexSite s{(int)v.at(0), u64(9), u64(10), u(8), 60u, 4u, 32u, false, 0u, b(11)};
            printf("loose_pays %%d\n", (int)loose_call_pays_rent(s, knobs, b(3), u(4), u64(5), u(6), u(7)));
        } else if (what == "loose_wants") {
            const IndexSite s{3, 0, 0, 2u, 60u, 4u, 32u, b(2), u(3), false};
            printf("loose_wants %%d\n", (int)loose_call_wants_index(s, u(0), u(1)));
        } else if (what == "runs") {
            knobs.use_filter = b(1), knobs.lazy = b(2);
            printf("runs %%d\n", (int)ladder_runs(u(0), knobs, b(3), u64(4)));
        } else if (what == "probed") {
            printf("probed %%d\n", (int)first_step_probed(b(0), b(1), u64(2), u(3), u(4), b(5)));
        } else if (what == "skips") {
            printf("skips %%d\n", (int)first_step_probe_skips(u(0), u(1)));
        } else if (what == "plans_now") {
            printf("plans_now %%d\n", (int)plans_later_now(b(0), u(1), u(2), u(3)));
        } else if (what == "sample") {
            printf("sample %%u\n", planner_sample(u(0)));
        } else if (what == "later") {
            const LaterSteps s = later_steps(ladder_from(2, v.size() - 2), u(0), u(1));
            printf("later %%d %%u\n", (int)s.any, (unsigned)s.last);
        } else if (what == "step_cost") {
            printf("step_cost %%.2f\n", step_cost(u(0), u(1)));
        } else if (what == "choose") {
            const LadderBounds l = ladder_from(4, u(3));
            const uint32_t ns = u(4 + u(3));
            std::vector<uint32_t> kth;
            for (uint32_t i = 0; i < ns; i++) kth.push_back(v.at(5 + u(3) + i) < 0 ? UINT32_MAX : u(5 + u(3) + i));
            const LaterChoice c = choose_later_steps(kth.data(), ns, l, u(1), u(2), u(0));
            printf("choose %%u %%.6f\n", c.mask, c.cost);
        } else if (what == "paid") {
            printf("paid %%d\n", (int)step_paid(u64(0), u(1), u(2)));
        } else if (what == "count_first") {
            printf("count_first %%d\n", (int)kth_count_first(u(0), u(1), ScanShape{u(2), u(3), u(4), u(5)}, knobs, u(6)));
        } else if (what == "hist_seed") {
            printf("hist_seed %%d\n", (int)kth_hist_seed(u(0), u(1), 256u, b(2)));
        } else if (what == "sample_tiles") {
            printf("sample_tiles %%u\n", kth_sample_tiles(b(0), u(1), u(2), u(3), u(4)));
        } else if (what == "scratch_rows") {
            printf("scratch_rows %%llu\n", (unsigned long long)kth_scratch_rows(b(0), u(1), u(2), u(3), u64(4)));
        } else if (what == "hist_groups") {
            printf("hist_groups %%u\n", kth_hist_groups(b(0), u(1), u(2), u(3), u(4)));
        } else if (what == "schedule") {
            const KthSchedule s = kth_schedule(u(0), u(1), b(2), u(3), b(4));
            printf("schedule");
            for (uint32_t i = 0; i < s.n; i++) {
                const KthScheduleStep &t = s.step[i];
                if (t.tile_begin == 0 && t.tile_end == 0) printf(" %%s", kind_name(t.kind));
                else printf(" %%s:%%u-%%u", kind_name(t.kind), t.tile_begin, t.tile_end);
            }
            printf("\n");
        } else if (what == "capacity") {
            printf("capacity %%u\n", kKthScheduleMax);
        } else {
            fprintf(stderr, "unknown question: %%s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
"""


def compiler():
    """the host compiler's path, or None where there is none"""
    return shutil.which(os.environ.get("CXX", "g++"))


def build(tmp):
    """compile the driver into directory `tmp`: the header with g++ alone, warnings as errors"""
    src = os.path.join(str(tmp), "kth_plan.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM % dict(header=HEADER))
    exe = os.path.join(str(tmp), "kth_plan")
    subprocess.run([compiler(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-o", exe, src], check=True, capture_output=True, text=True)
    return exe


def ask(exe, questions):
    """one answer per question, each as the list of words behind the question's name"""
    questions = list(questions)
    out = subprocess.run([exe], input="\n".join(questions) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(questions), (len(out), len(questions))
    answers = []
    for q, line in zip(questions, out):
        words = line.split()
        assert words[0] == q.split()[0], (q, line)
        answers.append(words[1:])
    return answers


def parse_schedule(words):
    """[(kind, begin, end)]; steps without a tile range: (kind, 0, 0)"""
    steps = []
    for w in words:
        kind, _, rng = w.partition(":")
        lo, _, hi = rng.partition("-") if rng else ("0", "", "0")
        steps.append((kind, int(lo), int(hi)))
    return steps

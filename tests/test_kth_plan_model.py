"""The decisions of the k-nearest path (smafa_amd/csrc/kth_plan.h) from the header compiled for the host: g++ alone, no HIP —
that the header compiles this way is part of the test (tests/kth_plan_model.py holds the driver).  Every expected value below
is worked by hand from the rules as the header's comments state them:

  * the ladder is {(cols - 1) / 6, 3 cols / 8}, cols = min(32, L) — 31 columns: 30 / 6 = 5 and 93 / 8 = 11; 32 and more: 31 / 6 = 5
    and 96 / 8 = 12 — and, at two words per plane (33..64 columns), a last step at 30 (two planes: 16) with a step at 17 in front
    of it for three planes and more from 2048 queries on;
  * an index that serves a bound at or above the first step's and below the call's own takes that bound as step 0 and every
    step at or below it leaves;
  * rent: queries x subjects x vectors x rate ms, 1.7e-12 under a fixed bound, 1.6e-11 without a usable one; the price is
    0.3 + blocks x subjects x 1e-7 ms, due from equality on;
  * blocks: width = max(2, floor((log2 n - 2) / bits)), bits 4.3 (aa), 2.0 (two planes) or 2.3; min(32, L / width):
      n = 1e4   log2 = 13.288: 11.288 / 4.3 = 2.6 -> 2 -> 30;  / 2.0 = 5.6 -> 5 -> 12;  / 2.3 = 4.9 -> 4 -> 15
      n = 1e7   log2 = 23.253: 21.253 / 4.3 = 4.9 -> 4 -> 15;  / 2.0 = 10.6 -> 10 -> 6; / 2.3 = 9.2 -> 9 -> 6
      n = 2^31 - 1  log2 just under 31: 29 / 4.3 = 6.7 -> 6 -> 10;  / 2.0 = 14.5 -> 14 -> 4;  / 2.3 = 12.6 -> 12 -> 5   (L = 60)
  * a later step costs 0.37 up to 3 cols / 8, 0.5 up to 17, 0.53 beyond, times the share still open, plus the open share left
    for the loose path; "no further step" costs 1.0 and a candidate must be strictly cheaper, masks tried in ascending order;
  * the schedule of a tightening scan: see SCHEDULES."""
import pytest

import kth_plan_model as model

pytestmark = pytest.mark.skipif(model.compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return model.build(tmp_path_factory.mktemp("kth_plan"))


def _check(exe, table):
    """table: [(question, expected answer as a string)]"""
    got = model.ask(exe, [q for q, _ in table])
    for (q, want), have in zip(table, got):
        assert " ".join(have) == want, (q, want, have)


def test_ladder(exe):
    _check(exe, [
        ("ladder 31 1 5 2048", "5 11"),
        ("ladder 31 1 2 10", "5 11"),
        ("ladder 60 2 2 2047", "5 12 16"),
        ("ladder 60 2 2 2048", "5 12 16"),  # (two planes: no step at 17)
        ("ladder 60 2 3 2047", "5 12 30"),
        ("ladder 60 2 3 2048", "5 12 17 30"),
        ("ladder 60 2 5 2047", "5 12 30"),
        ("ladder 60 2 5 2048", "5 12 17 30"),
        ("ladder 90 3 5 2048", "5 12"),
        ("ladder 150 5 5 2048", "5 12"),
        ("ladder 32 1 5 2048", "5 12"),
        ("ladder 32 2 5 2048", "5 12"),  # (two words need 33 columns)
        ("ladder 33 2 5 2047", "5 12 30"),
        ("ladder 33 2 5 2048", "5 12 17 30"),
        ("ladder 12 1 5 2048", "1 4"),  # 11 / 6, 36 / 8
    ])


def test_ladder_with_index(exe):
    _check(exe, [
        ("with_index 4 60 5 12 17 30", "0 5 12 17 30"),    # below the first step: no change
        ("with_index 5 60 5 12 17 30", "1 5 12 17 30"),    # equal to it: the same bounds, step 0 is the index's
        ("with_index 14 60 5 12 17 30", "1 14 17 30"),     # between two steps
        ("with_index 17 60 5 12 17 30", "1 17 30"),        # equal to a later step
        ("with_index 31 60 5 12 17 30", "1 31"),           # above the last
        ("with_index 60 60 5 12 17 30", "0 5 12 17 30"),   # at the call's own bound: no change
        ("with_index 14 12 5 12 17 30", "0 5 12 17 30"),   # above it
        ("with_index 11 12 5 12 17 30", "1 11 12 17 30"),  # just below it
    ])


def test_rent(exe):
    (fixed,), (loose,), (small,) = model.ask(exe, ["charge 10000 10000000 10 fixed", "charge 10000 10000000 10 loose", "charge 65 65536 2 fixed"])
    assert float(fixed) == pytest.approx(1.7, rel=1e-12)   # 1e4 x 1e7 x 10 x 1.7e-12
    assert float(loose) == pytest.approx(16.0, rel=1e-12)  # ... x 1.6e-11
    assert float(small) == pytest.approx(65 * 65536 * 2 * 1.7e-12, rel=1e-12)
    # six blocks over 1e7 subjects cost 0.3 + 6 x 1e7 x 1e-7 = 6.3 ms: a debt one charge (1.7 ms) below is not due, the price is
    price = 0.3 + 6.0 * 1e7 * 1.0e-7
    assert price == pytest.approx(6.3, rel=1e-12)
    _check(exe, [
        ("due %r 6 10000000" % (price - 1.7), "0"),
        ("due %r 6 10000000" % price, "1"),
        ("due 6.2999 6 10000000", "0"),
        ("due 6.3001 6 10000000", "1"),
        ("due 0.2999 0 10000000", "0"),
        ("due 0.3001 0 10000000", "1"),
    ])
    # three calls of 1.7 ms leave 5.1 < 6.3; the fourth pays
    _check(exe, [("due %r 6 10000000" % (1.7 * 3), "0"), ("due %r 6 10000000" % (1.7 * 4), "1")])


def test_index_blocks_wanted(exe):
    big = 2 ** 31 - 1
    _check(exe, [
        ("blocks 1 5 10000 60", "30"), ("blocks 1 5 10000000 60", "15"), ("blocks 1 5 %d 60" % big, "10"),
        ("blocks 0 2 10000 60", "12"), ("blocks 0 2 10000000 60", "6"), ("blocks 0 2 %d 60" % big, "4"),
        ("blocks 0 3 10000 60", "15"), ("blocks 0 3 10000000 60", "6"), ("blocks 0 3 %d 60" % big, "5"),
        ("blocks 1 5 10000 120", "32"),  # 120 / 2 = 60 blocks: at most 32
        ("blocks 1 5 16 60", "30"),      # log2 16 - 2 = 2: 0.47 -> width 2 all the same
    ])


def test_rent_eligibility(exe):
    # fixed_wants mode filter nq W thr0 L n min_rows current B failed
    _check(exe, [
        ("fixed_wants 2 1 65 2 5 60 65536 65536 0 0 0", "1"),
        ("fixed_wants 3 1 65 2 5 60 65536 65536 0 0 0", "1"),
        ("fixed_wants 1 1 65 2 5 60 65536 65536 0 0 0", "0"),  # mode 1 never builds
        ("fixed_wants 2 0 65 2 5 60 65536 65536 0 0 0", "0"),  # prefilter off
        ("fixed_wants 2 1 64 2 5 60 65536 65536 0 0 0", "0"),  # 64 queries: the few-query launch
        ("fixed_wants 2 1 65 5 5 150 65536 65536 0 0 0", "0"),  # five words per plane
        ("fixed_wants 2 1 65 4 5 128 65536 65536 0 0 0", "1"),
        ("fixed_wants 2 1 65 2 31 60 65536 65536 0 0 0", "1"),  # 32 blocks
        ("fixed_wants 2 1 65 2 32 60 65536 65536 0 0 0", "0"),  # 33
        ("fixed_wants 2 1 65 1 19 20 65536 65536 0 0 0", "1"),  # 20 blocks of one column
        ("fixed_wants 2 1 65 1 20 20 65536 65536 0 0 0", "0"),  # more blocks than columns
        ("fixed_wants 2 1 65 2 5 60 65535 65536 0 0 0", "0"),  # too few rows
        ("fixed_wants 2 1 65 2 5 60 2147483647 65536 0 0 0", "1"),
        ("fixed_wants 2 1 65 2 5 60 2147483648 65536 0 0 0", "0"),
        ("fixed_wants 2 1 65 2 5 60 65536 65536 1 6 0", "0"),  # a current index of six blocks serves bound 5
        ("fixed_wants 2 1 65 2 5 60 65536 65536 1 5 0", "1"),  # five do not
        ("fixed_wants 2 1 65 2 5 60 65536 65536 0 0 1", "1"),  # (a failed build still pays rent; the caller does not buy)
    ])
    # loose_pays mode filter lazy two_phase k nq limit first W n min_rows failed
    _check(exe, [
        ("loose_pays 3 1 1 1 1 65 60 5 2 65536 65536 0", "1"),
        ("loose_pays 2 1 1 1 1 65 60 5 2 65536 65536 0", "0"),  # mode 3 only
        ("loose_pays 3 0 1 1 1 65 60 5 2 65536 65536 0", "0"),
        ("loose_pays 3 1 0 1 1 65 60 5 2 65536 65536 0", "0"),
        ("loose_pays 3 1 1 0 1 65 60 5 2 65536 65536 0", "0"),
        ("loose_pays 3 1 1 1 0 65 60 5 2 65536 65536 0", "0"),  # no k
        ("loose_pays 3 1 1 1 1 64 60 5 2 65536 65536 0", "0"),
        ("loose_pays 3 1 1 1 1 65 5 5 2 65536 65536 0", "0"),   # the call's bound is the first step's
        ("loose_pays 3 1 1 1 1 65 6 5 2 65536 65536 0", "1"),
        ("loose_pays 3 1 1 1 1 65 60 5 5 65536 65536 0", "0"),
        ("loose_pays 3 1 1 1 1 65 60 5 2 65535 65536 0", "0"),
        ("loose_pays 3 1 1 1 1 65 60 5 2 2147483648 65536 0", "0"),
        ("loose_pays 3 1 1 1 1 65 60 5 2 65536 65536 1", "0"),  # a failed build: no rent until the store changes
    ])
    # loose_wants want first current B: the index must take at least the first step (first + 1 blocks) and not be there yet
    _check(exe, [("loose_wants 6 5 0 0", "1"), ("loose_wants 5 5 0 0", "0"), ("loose_wants 15 5 1 15", "0"), ("loose_wants 15 5 1 14", "1")])


def test_ladder_predicates(exe):
    _check(exe, [
        ("runs 1 1 1 1 16", "1"), ("runs 1 1 1 1 15", "0"), ("runs 0 1 1 1 16", "0"), ("runs 1 0 1 1 16", "0"), ("runs 1 1 0 1 16", "0"),
        ("runs 1 1 1 0 16", "0"),
        # probed laddered ladder_probe nq limit first index_first
        ("probed 1 1 2048 60 5 0", "1"), ("probed 0 1 2048 60 5 0", "0"), ("probed 1 0 2048 60 5 0", "0"), ("probed 1 1 2047 60 5 0", "0"),
        ("probed 1 1 2048 5 5 0", "0"), ("probed 1 1 2048 6 5 0", "1"), ("probed 1 1 2048 60 5 1", "0"),
        ("skips 15 256", "1"), ("skips 16 256", "0"),  # 15 x 16 = 240 < 256 = 16 x 16
        ("skips 0 256", "1"), ("skips 256 256", "0"),
        # plans_now planned open step n_steps
        ("plans_now 0 2048 0 2", "1"), ("plans_now 1 2048 0 2", "0"), ("plans_now 0 2047 0 2", "0"), ("plans_now 0 2048 1 2", "0"),
        ("plans_now 0 2048 2 4", "1"), ("plans_now 0 2048 3 4", "0"),
        ("sample 2048", "256"), ("sample 2047", "255"), ("sample 100000", "256"), ("sample 16", "2"),
        # later from limit bounds: the last step below the call's bound, and whether the first one is
        ("later 1 60 5 12 17 30", "1 3"), ("later 2 60 5 12 17 30", "1 3"), ("later 1 17 5 12 17 30", "1 1"), ("later 1 18 5 12 17 30", "1 2"),
        ("later 1 12 5 12 17 30", "0 1"), ("later 2 60 5 12", "0 2"),
        # a quarter where the next step is the one at 30, an eighth elsewhere
        ("paid 125 1000 30", "0"), ("paid 249 1000 30", "0"), ("paid 250 1000 30", "1"),
        ("paid 124 1000 17", "0"), ("paid 125 1000 17", "1"), ("paid 125 1000 0", "1"), ("paid 124 1000 0", "0"), ("paid 125 1000 29", "1"),
    ])


def test_choose_later_steps(exe):
    none, ladder4, ladder3 = "-1", "4 5 12 17 30", "3 5 12 30"
    _check(exe, [
        # the cost classes on both sides of 3 cols / 8 (32 columns: 12; 31: 11) and of 17
        ("step_cost 12 32", "0.37"), ("step_cost 13 32", "0.50"), ("step_cost 11 31", "0.37"), ("step_cost 12 31", "0.50"),
        ("step_cost 17 32", "0.50"), ("step_cost 18 32", "0.53"), ("step_cost 30 32", "0.53"),
        # two later steps, at 17 (0.5) and 30 (0.53), eight sample queries.  Everybody within 17: {17} 0.5 + 0; {30} 0.53; both
        # 0.5 + 0 x 0.53 + 0 = 0.5, a tie that the earlier mask keeps
        ("choose 32 2 3 %s 8 %s" % (ladder4, " ".join(["15"] * 8)), "1 0.500000"),
        # everybody between 18 and 30: {17} 0.5 + 1; {30} 0.53 + 0; both 0.5 + 0.53 + 0
        ("choose 32 2 3 %s 8 %s" % (ladder4, " ".join(["25"] * 8)), "2 0.530000"),
        # nobody within 30: {17} 1.5, {30} 1.53, both 2.03: no step, 1.0
        ("choose 32 2 3 %s 8 %s" % (ladder4, " ".join([none] * 8)), "0 1.000000"),
        # half within 17, a quarter within 30, a quarter nowhere: {17} 0.5 + 0.5 = 1.0 (not below 1.0); {30} 0.53 + 0.25 = 0.78;
        # both 0.5 + 0.5 x 0.53 + 0.25 = 1.015
        ("choose 32 2 3 %s 8 15 15 15 15 25 25 %s %s" % (ladder4, none, none), "2 0.780000"),
        # exactly half within 17 and nobody else within 30: {17} ties with "no step" at 1.0 and loses
        ("choose 32 2 3 %s 8 15 15 15 15 %s" % (ladder4, " ".join([none] * 4)), "0 1.000000"),
        # later steps at 12 (0.37) and 30 (0.53); seven of eight within 12, one within 30: {12} 0.37 + 0.125 = 0.495; {30} 0.53;
        # both 0.37 + 0.125 x 0.53 + 0 = 0.43625
        ("choose 32 1 2 %s 8 10 10 10 10 10 10 10 25" % ladder3, "3 0.436250"),
        # 31 columns: 12 is past 3 x 31 / 8 = 11 and costs 0.5: {12} 0.625, {30} 0.53, both 0.5 + 0.06625 = 0.56625
        ("choose 31 1 2 %s 8 10 10 10 10 10 10 10 25" % ladder3, "2 0.530000"),
        # a distance equal to the bound finishes there
        ("choose 32 2 3 %s 4 17 17 17 17" % ladder4, "1 0.500000"),
        ("choose 32 2 3 %s 4 18 18 18 18" % ladder4, "2 0.530000"),
        # one later step, the one at 30: everybody within it 0.53, nobody 1.53 -> none
        ("choose 32 2 2 %s 8 %s" % (ladder3, " ".join(["25"] * 8)), "1 0.530000"),
        ("choose 32 2 2 %s 8 %s" % (ladder3, " ".join([none] * 8)), "0 1.000000"),
        # ... and below half of the sample it does not pay: 3 of 8: 0.53 + 0.625; 4 of 8: 0.53 + 0.5 = 1.03; 5 of 8: 0.905
        ("choose 32 2 2 %s 8 25 25 25 25 %s" % (ladder3, " ".join([none] * 4)), "0 1.000000"),
        ("choose 32 2 2 %s 8 25 25 25 25 25 %s" % (ladder3, " ".join([none] * 3)), "1 0.905000"),
    ])


def test_count_first_and_sample(exe):
    _check(exe, [
        # count_first k count_first_k P PQ W L thr0: k at least count_first_k and a bound level 1 does not prune at (32 columns: 8 up)
        ("count_first 3 3 5 5 2 60 60", "1"), ("count_first 2 3 5 5 2 60 60", "0"), ("count_first 3 3 5 5 2 60 7", "0"),
        ("count_first 3 3 5 5 2 60 8", "1"), ("count_first 2 2 2 3 1 31 31", "1"),
        ("hist_seed 2 255 1", "1"), ("hist_seed 1 60 1", "0"), ("hist_seed 2 256 1", "0"), ("hist_seed 2 60 0", "0"),
        # sample_tiles count_first div min_tiles n_tiles k
        ("sample_tiles 1 32 4096 8192 5", "256"),
        ("sample_tiles 0 32 4096 8192 5", "0"),  # not counting first
        ("sample_tiles 1 0 4096 8192 5", "0"),   # SMAFA_KTH_SAMPLE=0
        ("sample_tiles 1 32 4096 4095 5", "0"),  # one tile below the minimum
        ("sample_tiles 1 32 4096 4096 5", "128"),
        ("sample_tiles 1 32 1 31 5", "0"),       # fewer tiles than the divisor
        ("sample_tiles 1 32 1 32 5", "1"),
        ("sample_tiles 1 16 8 41 128", "2"),     # 4 k = 512 = the sample's rows
        ("sample_tiles 1 16 8 41 129", "0"),     # 4 k = 516
        ("sample_tiles 1 32 1 32 64", "1"), ("sample_tiles 1 32 1 32 65", "0"),
        ("sample_tiles 1 8 8 41 5", "5"), ("sample_tiles 1 2 8 41 5", "20"), ("sample_tiles 1 2 8 161 5", "80"), ("sample_tiles 1 2 8 5 5", "0"),
        # scratch_rows count_first sample_tiles nq k cap: none when counting everything first; else max(2 cap, min(nq x per query,
        # 2^27)), 128 per query, 16 k + 128 with a sample
        ("scratch_rows 1 0 75 5 4194304", "0"),
        ("scratch_rows 0 0 75 1 100", "9600"), ("scratch_rows 0 0 75 1 4800", "9600"), ("scratch_rows 0 0 75 1 4801", "9602"),
        ("scratch_rows 1 20 75 5 100", "15600"),  # 75 x 208
        ("scratch_rows 0 0 2000000 1 100", "134217728"),  # 2.56e8 capped at 2^27
        # hist_groups counting tiles n_chunks n_cu override: the seed form 1; counting min(4-tile steps, ceil(8 n_cu / chunks)), at least 1
        ("hist_groups 0 80 3 256 0", "1"), ("hist_groups 1 80 3 256 0", "20"), ("hist_groups 1 80 3 256 2", "2"), ("hist_groups 1 80 3 256 40", "20"),
        ("hist_groups 1 8192 313 256 0", "7"),  # ceil(2048 / 313)
        ("hist_groups 1 1 3 256 0", "1"), ("hist_groups 1 5 3 256 0", "2"),
    ])


# ---- the schedule ---------------------------------------------------------------------------------------------------------
# Worked by hand.  Z = ZeroCounts (k >= 2 only), the seed: SS over min(4, n) tiles for k = 1 and over 1 tile (followed by Z:
# its pairs are counted again) for k >= 2, or SH over min(4, n) tiles with the histogram seed; then tightening launches over
# segments of 4 tiles growing 8x (4, 32, 256; with the histogram seed from 32) — A, appending, or C where everything is counted
# first, which ends B XC over every tile; all others end F.  With a sample of s tiles only [0, s) is walked that way (the
# histogram counts it whole: MH), then B, A over the rest in segments of 3 s growing 4x, B, XS over [0, s), F.
# (n_tiles, form, histogram seed switch) -> steps; forms: "k1", "k2" (k = 2, appending), "cf" (k = 5 counting first, no sample),
# "s8" / "s2" (k = 5 counting first, SMAFA_KTH_SAMPLE = 8 / 2 under SMAFA_KTH_SAMPLE_MIN_TILES=8: no sample below 8 tiles)
SCHEDULES = {
    (1, "k1"): "SS:0-1 A:0-1 F",
    (4, "k1"): "SS:0-4 A:0-4 F",
    (5, "k1"): "SS:0-4 A:0-4 A:4-5 F",
    (41, "k1"): "SS:0-4 A:0-4 A:4-36 A:36-41 F",
    (161, "k1"): "SS:0-4 A:0-4 A:4-36 A:36-161 F",
    (1, "k2", 0): "Z SS:0-1 Z A:0-1 F",
    (4, "k2", 0): "Z SS:0-1 Z A:0-4 F",
    (5, "k2", 0): "Z SS:0-1 Z A:0-4 A:4-5 F",
    (41, "k2", 0): "Z SS:0-1 Z A:0-4 A:4-36 A:36-41 F",
    (161, "k2", 0): "Z SS:0-1 Z A:0-4 A:4-36 A:36-161 F",
    (1, "k2", 1): "Z SH:0-1 A:0-1 F",
    (4, "k2", 1): "Z SH:0-4 A:0-4 F",
    (5, "k2", 1): "Z SH:0-4 A:0-5 F",
    (41, "k2", 1): "Z SH:0-4 A:0-32 A:32-41 F",
    (161, "k2", 1): "Z SH:0-4 A:0-32 A:32-161 F",
    (1, "cf", 0): "Z SS:0-1 Z C:0-1 B XC:0-1",
    (4, "cf", 0): "Z SS:0-1 Z C:0-4 B XC:0-4",
    (5, "cf", 0): "Z SS:0-1 Z C:0-4 C:4-5 B XC:0-5",
    (41, "cf", 0): "Z SS:0-1 Z C:0-4 C:4-36 C:36-41 B XC:0-41",
    (161, "cf", 0): "Z SS:0-1 Z C:0-4 C:4-36 C:36-161 B XC:0-161",
    (1, "cf", 1): "Z SH:0-1 C:0-1 B XC:0-1",
    (4, "cf", 1): "Z SH:0-4 C:0-4 B XC:0-4",
    (5, "cf", 1): "Z SH:0-4 C:0-5 B XC:0-5",
    (41, "cf", 1): "Z SH:0-4 C:0-32 C:32-41 B XC:0-41",
    (161, "cf", 1): "Z SH:0-4 C:0-32 C:32-161 B XC:0-161",
    (41, "s8", 0): "Z SS:0-1 Z C:0-4 C:4-5 B A:5-20 A:20-41 B XS:0-5 F",       # sample 5; the rest from 15 tiles
    (41, "s8", 1): "Z MH:0-5 B A:5-20 A:20-41 B XS:0-5 F",
    (41, "s2", 0): "Z SS:0-1 Z C:0-4 C:4-20 B A:20-41 B XS:0-20 F",            # sample 20; the rest from 60
    (41, "s2", 1): "Z MH:0-20 B A:20-41 B XS:0-20 F",
    (161, "s8", 0): "Z SS:0-1 Z C:0-4 C:4-20 B A:20-80 A:80-161 B XS:0-20 F",  # sample 20; 60, then 240
    (161, "s8", 1): "Z MH:0-20 B A:20-80 A:80-161 B XS:0-20 F",
    (161, "s2", 0): "Z SS:0-1 Z C:0-4 C:4-36 C:36-80 B A:80-161 B XS:0-80 F",  # sample 80; the rest from 240
    (161, "s2", 1): "Z MH:0-80 B A:80-161 B XS:0-80 F",
}
for _n in (1, 4, 5):  # below 8 tiles there is no sample: the counting-first form as it is
    for _s in ("s8", "s2"):
        for _h in (0, 1):
            SCHEDULES[_n, _s, _h] = SCHEDULES[_n, "cf", _h]
for _n in (1, 4, 5, 41, 161):  # k = 1 has no histogram seed: the switch changes nothing
    SCHEDULES[_n, "k1", 0] = SCHEDULES[_n, "k1", 1] = SCHEDULES.pop((_n, "k1"))

FORMS = {"k1": (1, 0, 0), "k2": (2, 0, 0), "cf": (5, 1, 0), "s8": (5, 1, 8), "s2": (5, 1, 2)}  # k, counting first, SMAFA_KTH_SAMPLE
MIN_TILES = 8


def _schedules(exe, cases):
    """cases: [(n_tiles, form, hist switch)] -> [(sample_tiles, steps)] through kth_sample_tiles, kth_hist_seed and kth_schedule"""
    first = []
    for n, form, hist in cases:
        k, cf, div = FORMS[form]
        first += ["sample_tiles %d %d %d %d %d" % (cf, div, MIN_TILES, n, k), "hist_seed %d 60 %d" % (k, hist)]
    a = model.ask(exe, first)
    samples, seeds = [int(x[0]) for x in a[0::2]], [int(x[0]) for x in a[1::2]]
    second = ["schedule %d %d %d %d %d" % (n, FORMS[form][0], FORMS[form][1], s, h) for (n, form, _), s, h in zip(cases, samples, seeds)]
    return list(zip(samples, [model.parse_schedule(w) for w in model.ask(exe, second)]))


COUNTING, APPENDING = ("MH", "C", "A"), ("A", "XS")


def _structure(n, form, sample, steps, capacity):
    k, cf, _ = FORMS[form]
    kinds = [s[0] for s in steps]
    where = (n, form, sample, steps)
    assert len(steps) <= capacity, where
    # every tile is counted exactly once, by segments that are contiguous and ascending — behind the last ZeroCounts (the seed
    # scan's own tiles are counted again after the ZeroCounts that follows it)
    last_zero = max([i for i, kd in enumerate(kinds) if kd == "Z"], default=-1)
    assert (last_zero >= 0) == (k >= 2), where
    if "SS" in kinds and k >= 2:
        assert kinds[kinds.index("SS") + 1] == "Z", where
    at = 0
    for i, (kd, lo, hi) in enumerate(steps):
        if kd in COUNTING:
            assert i > last_zero and lo == at and hi > lo, where
            at = hi
    assert at == n, where
    seeds = [s for s in steps if s[0] in ("SS", "SH", "MH")]
    assert len(seeds) == 1 and seeds[0][1] == 0, where  # one seed, from tile 0
    if sample:
        # ... and appended exactly once: the rest of the store while it is counted, then the sample's own tiles
        spans = sorted((lo, hi) for kd, lo, hi in steps if kd in APPENDING)
        assert spans[0] == (0, sample) and [lo for lo, _ in spans[1:]] == [hi for _, hi in spans[:-1]] and spans[-1][1] == n, where
        assert kinds.count("B") == 2 and kinds[-3:] == ["B", "XS", "F"], where
    if cf and not sample:  # the one form without a filter pass: the exact bounds, then every tile straight into the caller's list
        assert kinds[-2:] == ["B", "XC"] and steps[-1][1:] == (0, n) and "F" not in kinds and "A" not in kinds, where
    else:
        assert kinds[-1] == "F" and kinds.count("F") == 1 and "XC" not in kinds, where


def test_schedule_cases(exe):
    cases = sorted(SCHEDULES)
    assert len(cases) == 5 * 5 * 2
    capacity = int(model.ask(exe, ["capacity"])[0][0])
    for (n, form, hist), (sample, steps) in zip(cases, _schedules(exe, cases)):
        want = model.parse_schedule(SCHEDULES[n, form, hist].split())
        assert steps == want, (n, form, hist, sample, steps, want)
        _structure(n, form, sample, steps, capacity)


def test_schedule_structure_at_every_size(exe):
    capacity = int(model.ask(exe, ["capacity"])[0][0])
    assert capacity == 32
    forms = {"k1": (1, 0, 0), "k2": (2, 0, 0), "cf": (5, 1, 0), "d2": (5, 1, 2), "d8": (5, 1, 8), "d32": (5, 1, 32)}
    FORMS.update(forms)
    cases = [(n, form, hist) for n in range(1, 601) for form in forms for hist in (0, 1)]
    sampled = 0
    for (n, form, hist), (sample, steps) in zip(cases, _schedules(exe, cases)):
        _structure(n, form, sample, steps, capacity)
        sampled += sample != 0
    assert sampled == 2 * sum(1 for n in range(8, 601) for d in (2, 8, 32) if n // d >= 1)
    # the largest store (2^24 wave tiles) at the sample sizes with the most segments: within the capacity, every tile once
    big = 1 << 24
    words = model.ask(exe, ["schedule %d 5 1 %d %d" % (big, s, h) for s in (0, 1, 2, big // 32, big // 2) for h in (0, 1)] +
                      ["schedule %d 1 0 0 0" % big, "schedule %d 2 0 0 1" % big])
    lengths = []
    for i, w in enumerate(words):
        steps = model.parse_schedule(w)
        form, sample = ("k1", 0) if i == 10 else ("k2", 0) if i == 11 else ("d32", (0, 1, 2, big // 32, big // 2)[i // 2])
        _structure(big, form, sample, steps, capacity)
        lengths.append(len(steps))
    # the longest: a sample of one tile, no histogram: Z SS Z C B, then appending segments of 3 x 4^j tiles from tile 1 on, which
    # end at tile 4^j: 12 of them reach 4^12 = 2^24; B XS F
    assert lengths[2] == 5 + 12 + 3 and max(lengths) == 20, lengths

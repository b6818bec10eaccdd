"""The self-join's piece-size rule (engine.h: join_piece_rule; self_join.hip.h: join_pass), from the header compiled for the host.

After a piece's scan the host knows its exact row count.  A count the scratch list held: the piece is taken.  A count above
the capacity but within the ceiling (SMAFA_JOIN_SCRATCH_MAX): the list grows to the count and the same rows are scanned again.
A count above the ceiling: the piece is cut to max(64, ((rows / 2 + 63) / 64) * 64) rows, and a piece of 64 rows or fewer fails.
A reduced piece size doubles back, at most to the block size, after a taken piece whose count x 4 is below the ceiling.  The
expected values below are worked by hand from these rules."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, CAP, CEILING = 65536, 4194304, 1000000

# (count, capacity, ceiling, rows, piece, block) -> (verdict, rows per scan from here on)
CASES = [
    ((1000, 4096, CEILING, BLOCK, BLOCK, BLOCK), ("take", BLOCK)),        # under the capacity
    ((4096, 4096, CEILING, BLOCK, BLOCK, BLOCK), ("take", BLOCK)),        # ... and exactly at it
    ((0, 4096, CEILING, 100, BLOCK, BLOCK), ("take", BLOCK)),             # no row at all
    ((500000, 4096, CEILING, BLOCK, BLOCK, BLOCK), ("grow", BLOCK)),      # over the capacity, under the ceiling
    ((CEILING, 4096, CEILING, BLOCK, BLOCK, BLOCK), ("grow", BLOCK)),     # ... and exactly at it
    ((500000, 4096, CEILING, 8192, 8192, BLOCK), ("grow", 8192)),         # (a reduced piece size is kept)
    ((2000000, 4096, CEILING, 65536, BLOCK, BLOCK), ("halve", 32768)),    # over the ceiling: 65 536 / 2
    ((2000000, 4096, CEILING, 130, BLOCK, BLOCK), ("halve", 128)),        # 65 rows, rounded up to two chunks of 64
    ((2000000, 4096, CEILING, 65, BLOCK, BLOCK), ("halve", 64)),          # 32 rows, rounded up to one chunk
    ((2000000, 4096, CEILING, 64, 64, BLOCK), ("fail", 64)),              # one chunk cannot be cut
    ((2000000, CAP, CEILING, 65536, BLOCK, BLOCK), ("take", BLOCK)),      # (a list that is larger than the ceiling already holds it)
    # the double-back below, at and above a quarter of the ceiling — with the piece at the block size there is nothing to double
    ((249999, CAP, CEILING, BLOCK, BLOCK, BLOCK), ("take", BLOCK)),
    ((250000, CAP, CEILING, BLOCK, BLOCK, BLOCK), ("take", BLOCK)),
    ((250001, CAP, CEILING, BLOCK, BLOCK, BLOCK), ("take", BLOCK)),
    # ... and with a reduced piece
    ((249999, CAP, CEILING, 16384, 16384, BLOCK), ("take", 32768)),
    ((250000, CAP, CEILING, 16384, 16384, BLOCK), ("take", 16384)),
    ((250001, CAP, CEILING, 16384, 16384, BLOCK), ("take", 16384)),
    ((0, CAP, CEILING, 40000, 40000, BLOCK), ("take", BLOCK)),            # doubled, but never past the block size
    ((10, CAP, CEILING, 64, 64, 128), ("take", 128)),
]


def test_piece_rule_table(tmp_path):
    src = tmp_path / "rule.cpp"
    rows = ", ".join("{%s}" % ", ".join("%dull" % v for v in args) for args, _ in CASES)
    src.write_text(
        '#include <cstdio>\n#include "%s"\n'
        "int main() {\n"
        "    const unsigned long long cases[][6] = {%s};\n"
        "    for (const auto &c : cases) {\n"
        "        const smafa::PieceRule r = smafa::join_piece_rule(c[0], c[1], c[2], c[3], c[4], c[5]);\n"
        '        printf("%%s %%llu\\n", r.verdict == smafa::kPieceTake ? "take" : r.verdict == smafa::kPieceGrow ? "grow" :\n'
        '               r.verdict == smafa::kPieceHalve ? "halve" : "fail", (unsigned long long)r.piece);\n'
        "    }\n"
        "}\n" % (os.path.join(ROOT, "smafa_amd", "csrc", "engine.h"), rows))
    exe = str(tmp_path / "rule")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-o", exe, str(src)], check=True, capture_output=True, text=True)
    out = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = [(v, int(p)) for v, p in out]
    assert len(got) == len(CASES)
    for (args, want), have in zip(CASES, got):
        assert have == want, (args, want, have)

"""Host check of csrc/row_ranges.h: the one function that sizes the grid of every persistent row-streaming launch gives, for every
row count, tile height, blocks-per-CU factor and CU count in use, the (grid, rows per block) of the expressions the launchers spelled
out one by one before it existed -- and the ranges cover all rows with no empty block.  A plain C++ program, no GPU."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "row_ranges.h"

// the launchers' own spelling, kept literally
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

int main() {
    const int ROWS_SET[3] = {16, 32, 64}, PER_CU[3] = {1, 2, 4}, CUS[4] = {256, 255, 248, 1};
    uint64_t h_helper = 1469598103934665603ull, h_literal = 1469598103934665603ull;
    long uncovered = 0, combos = 0;
    auto mix = [](uint64_t& h, int grid, int rpb) {
        h = (h ^ (uint64_t)(uint32_t)grid) * 1099511628211ull;
        h = (h ^ (uint64_t)(uint32_t)rpb) * 1099511628211ull;
    };
    for (int ri = 0; ri < 3; ++ri)
        for (int pi = 0; pi < 3; ++pi)
            for (int ci = 0; ci < 4; ++ci)
                for (int rows = 1; rows <= 70000; ++rows) {
                    const int ROWS = ROWS_SET[ri], per_cu = PER_CU[pi], cus = CUS[ci];
                    const RowRanges r = row_ranges(rows, ROWS, cus, per_cu);
                    mix(h_helper, r.grid, r.rpb);
                    const int tiles = cdiv(rows, ROWS);
                    const int want = per_cu * cus;
                    const int blocks = tiles < want ? tiles : want;
                    const int rpb = cdiv(cdiv(rows, blocks), ROWS) * ROWS;
                    const int grid = cdiv(rows, rpb);
                    mix(h_literal, grid, rpb);
                    const bool covered = (long)r.grid * r.rpb >= rows && (long)(r.grid - 1) * r.rpb < rows;
                    if (!covered || r.rpb % ROWS != 0 || r.grid < 1 || r.grid > r.blocks || r.blocks != blocks) ++uncovered;
                    ++combos;
                }
    printf("helper %016llx literal %016llx uncovered %ld combos %ld\n", (unsigned long long)h_helper, (unsigned long long)h_literal, uncovered, combos);
    return 0;
}
"""


def test_row_ranges_match_the_launchers_expressions(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "row_ranges_walk.cpp"
    exe = tmp_path / "row_ranges_walk"
    src.write_text(PROGRAM)
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I" + os.path.join(REPO, "contrastive_lift_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "helper" and words[2] == "literal" and words[4] == "uncovered" and words[6] == "combos", r.stdout
    assert int(words[7]) == 70000 * 3 * 3 * 4                  # every combination was walked
    assert words[1] == words[3], r.stdout                      # same (grid, rows per block) as the literal expressions, everywhere
    assert int(words[5]) == 0, r.stdout                        # grid * rpb >= rows, (grid - 1) * rpb < rows, rpb a multiple of ROWS


def test_row_ranges_of_nothing_is_no_blocks(tmp_path):
    """rows <= 0 never reaches a launch (the entry points return first); the function answers it with zeros instead of dividing by zero."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "row_ranges_zero.cpp"
    exe = tmp_path / "row_ranges_zero"
    src.write_text('#include <cstdio>\n#include "row_ranges.h"\nint main() { const RowRanges r = row_ranges(0, 32, 256); '
                   'printf("%d %d %d\\n", r.blocks, r.rpb, r.grid); return 0; }\n')
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I" + os.path.join(REPO, "contrastive_lift_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["0", "0", "0"]

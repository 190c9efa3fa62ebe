// row_ranges.h -- how a persistent row-streaming launch divides its rows among blocks.  Plain C++ (nothing from HIP), so that a host program
// can include it: tests/test_row_ranges_host.py walks it against the expressions the launchers used to spell out one by one.
#pragma once

struct RowRanges {
    int blocks;   // blocks the rows are balanced over: one per ROWS-row tile, at most per_cu per CU
    int rpb;      // rows per block, a multiple of ROWS
    int grid;     // blocks that own at least one row (<= blocks): what most launchers launch
};

// `rows` rows in tiles of ROWS, over at most per_cu * cus blocks (no rows: no blocks -- the launchers return before they get here)
static inline RowRanges row_ranges(long rows, int ROWS, int cus, int per_cu = 1) {
    const long tiles = (rows + ROWS - 1) / ROWS, want = (long)per_cu * cus;
    RowRanges r = {0, 0, 0};
    if (rows <= 0 || want <= 0) return r;
    r.blocks = (int)(tiles < want ? tiles : want);
    r.rpb = (int)(((rows + r.blocks - 1) / r.blocks + ROWS - 1) / ROWS) * ROWS;
    r.grid = (int)((rows + r.rpb - 1) / r.rpb);
    return r;
}

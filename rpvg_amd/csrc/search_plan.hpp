// The host plan of the diploid search (bounded_search.hip): which kernel every matrix of a batch gets and the work items of
// the table path — a pure computation on the matrices' sizes, plain C++17, so that a CPU test reaches every decision
// (tests/cpp/search_plan_check.cpp).  queuePairSearch uploads the plan and launches what it says.
#ifndef RPVG_SEARCH_PLAN_HPP
#define RPVG_SEARCH_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif

namespace rpvg_search {

constexpr uint32_t kChunkRows = 1024;            // rows of a work item of the table path
constexpr int kTileA = 4;                        // first columns of a work item of pairTableKernel
constexpr uint32_t kSmallRows = 512;             // matrices with at most this many rows: the small sequential kernel
constexpr uint32_t kTileBlock = 256;             // lanes of a workgroup of pairTile2Kernel
constexpr uint32_t kTileMaxColumns = 1024;       // wider matrices keep the sequential search (their pair tables would not fit either)
constexpr uint32_t kTile2BufferDoubles = 3 * 1024;  // a staging buffer of pairTile2Kernel; two of them: 48 KB (three workgroups per CU)
constexpr uint64_t kTableBudget = 1ull << 28;    // doubles of partial pair sums (2 GiB)
constexpr double kTableMinWork = 65536.0;        // rows x columns from which a matrix takes the sequential route's table path

RPVG_PLAN_FN uint32_t tileColumns(const uint32_t G) { return (G + 3) / 4; }
RPVG_PLAN_FN uint32_t tileCount(const uint32_t G) { return tileColumns(G) * (tileColumns(G) + 1) / 2; }
// row slices of a chunk: lanes left over by the tiles
RPVG_PLAN_FN uint32_t tileSlices(const uint32_t G) { return tileCount(G) <= kTileBlock ? kTileBlock / tileCount(G) : 1u; }
// Rows per staged block: a compile-time constant, so that the eight values of a row sit at immediate offsets from one address
// per side (a stride in a register cost nine address additions and nine increments per row next to the 36 FP64 instructions);
// even (a lane loads two).  The largest of the menu whose block fits a buffer.
RPVG_PLAN_FN uint32_t tileSubRows(const uint32_t ncols) {
    const uint32_t fit = (kTile2BufferDoubles - ncols / 2) / (ncols + 2);
    return fit >= 126 ? 126u : fit >= 94 ? 94u : fit >= 46 ? 46u : fit >= 30 ? 30u : fit >= 14 ? 14u : fit >= 6 ? 6u : 2u;
}

// The tiles of a matrix cut into the ranges of its work items: 256 at a time, and what is left so that tiles x slices fills
// the workgroup — one more slice for as many tiles as fit then, the rest of the tiles in an item of their own (its lanes walk
// 1 / slices of the rows each) — whenever that walks at least a tenth fewer rows per lane than one item with the slices that fit.
inline void planTileRanges(const uint32_t tiles, std::vector<std::pair<uint32_t, uint32_t> > * ranges) {
    uint32_t t0 = 0, left = tiles;
    while (left > 0) {
        if (left >= kTileBlock) {
            ranges->emplace_back(t0, kTileBlock);
            t0 += kTileBlock;
            left -= kTileBlock;
            continue;
        }
        const uint32_t slices = kTileBlock / left;
        const uint32_t more = kTileBlock / (slices + 1), rest = left - more;
        const double one = 1.0 / slices, two = 1.0 / (slices + 1) + 1.0 / (kTileBlock / rest);
        if (two < 0.9 * one) {
            ranges->emplace_back(t0, more);
            t0 += more;
            left = rest;
        } else {
            ranges->emplace_back(t0, left);
            left = 0;
        }
    }
}

// What the environment may change (bounded_search.hip reads it, per call; the plan never does)
struct PairSearchKnobs {
    int tiles_wanted = 2;                    // RPVG_HIP_PAIR_TILES: 0 keeps the sequential search with its table path (A/B)
    double table_min_work = kTableMinWork;   // RPVG_HIP_TABLE_MIN_WORK (the sequential route; tests use 0)
    uint32_t chunk_rows = kChunkRows;        // RPVG_HIP_PAIR_CHUNK_ROWS (the tile kernel; the tests cut small matrices into several chunks)
};

struct PairSearchPlan {
    bool pair_tiles = false;         // the table part goes to pairTile2Kernel (else pairTableKernel)
    uint32_t chunk_rows = kChunkRows;
    std::vector<uint32_t> order;     // [table | medium | small], each part expensive first (R G^2, ties by index)
    uint32_t num_big = 0, num_medium = 0;
    std::vector<uint64_t> col_off, pair_cap_off;  // [M + 1] prefixes of G and of G (G + 1) / 2
    // work items of the table part: with tiles (matrix, first tile | (tiles - 1) << 16, chunk), else (matrix, first column, chunk)
    std::vector<uint32_t> item_matrix, item_col, item_chunk;
    // [M] offsets of a table matrix's [chunk][G] partial column sums and [chunk][G][G] partial pair sums (0 for the others)
    std::vector<uint64_t> big_col_part_off, big_pair_part_off;
    uint64_t col_part_total = 0, pair_part_total = 0;
};

// Big matrices take the table path: every pair evaluated in parallel by (tiles or columns, row chunk) workgroups, then one
// resolving workgroup; the rest take the search inside one workgroup.  With tiles — the default for a threshold that is a
// ratio <= 1 — every matrix of at most kTileMaxColumns columns whose sums fit the budget is a table matrix; on the sequential
// route the table matrices are a prefix of the cost order.  A ratio above 1: no table (the prefix-maximum form of the rule
// does not hold).
inline PairSearchPlan planPairSearch(const uint64_t * num_rows, const uint32_t * num_cols, const uint32_t M, const double min_rel_likelihood,
                                     const PairSearchKnobs & knobs) {
    PairSearchPlan p;
    p.col_off.assign(M + 1, 0);
    p.pair_cap_off.assign(M + 1, 0);
    for (uint32_t m = 0; m < M; ++m) {
        const uint64_t G = num_cols[m];
        p.col_off[m + 1] = p.col_off[m] + G;
        p.pair_cap_off[m + 1] = p.pair_cap_off[m] + G * (G + 1) / 2;
    }
    std::vector<uint32_t> cost_order(M);
    std::iota(cost_order.begin(), cost_order.end(), 0);
    std::sort(cost_order.begin(), cost_order.end(), [&](uint32_t x, uint32_t y) {
        const double wx = static_cast<double>(num_rows[x]) * num_cols[x] * num_cols[x];
        const double wy = static_cast<double>(num_rows[y]) * num_cols[y] * num_cols[y];
        return wx != wy ? wx > wy : x < y;
    });
    p.pair_tiles = knobs.tiles_wanted != 0 && min_rel_likelihood <= 1;
    p.chunk_rows = p.pair_tiles ? knobs.chunk_rows : kChunkRows;
    const double table_min_work = min_rel_likelihood > 1 ? 1e300 : knobs.table_min_work;
    p.big_col_part_off.assign(M, 0);
    p.big_pair_part_off.assign(M, 0);
    std::vector<uint32_t> medium, small;
    std::vector<std::pair<uint32_t, uint32_t> > ranges;
    bool table_closed = false;
    for (const uint32_t m : cost_order) {
        const uint64_t R = num_rows[m], G = num_cols[m];
        const uint64_t chunks = (R + p.chunk_rows - 1) / p.chunk_rows;
        const bool fits = p.pair_part_total + chunks * G * G <= kTableBudget;
        const bool takes_table = p.pair_tiles ? (G <= kTileMaxColumns && fits)
                                              : (!table_closed && static_cast<double>(R) * G >= table_min_work && fits);
        if (!takes_table) {
            table_closed = true;
            (R > kSmallRows ? medium : small).push_back(m);
            continue;
        }
        p.order.push_back(m);
        p.big_col_part_off[m] = p.col_part_total;
        p.big_pair_part_off[m] = p.pair_part_total;
        p.col_part_total += chunks * G;
        p.pair_part_total += chunks * G * G;
        ranges.clear();
        if (p.pair_tiles) planTileRanges(tileCount(static_cast<uint32_t>(G)), &ranges);
        else for (uint32_t a = 0; a < G; a += kTileA) ranges.emplace_back(a, 1u);
        for (uint32_t c = 0; c < chunks; ++c) {
            for (const auto & range : ranges) {
                p.item_matrix.push_back(m);
                p.item_col.push_back(range.first | ((range.second - 1) << 16));
                p.item_chunk.push_back(c);
            }
        }
    }
    p.num_big = static_cast<uint32_t>(p.order.size());
    p.num_medium = static_cast<uint32_t>(medium.size());
    p.order.insert(p.order.end(), medium.begin(), medium.end());
    p.order.insert(p.order.end(), small.begin(), small.end());
    return p;
}

}  // namespace rpvg_search

#endif

// The decisions of the minimum path cover (`-i strains`) as pure computations on sizes: which of the two routes a listed cluster
// takes — one workgroup (path_cover.hip) or the whole GPU, a cluster at a time (path_cover_grid.hip) —, the limits of either, how
// the host drives the rounds of the grid route, and the sizes of that route's scratch.  Plain C++17, no HIP types, no getenv: a
// CPU test reaches every decision (tests/cpp/cover_plan_check.cpp).  This is the only place that knows these numbers.
#ifndef RPVG_COVER_PLAN_HPP
#define RPVG_COVER_PLAN_HPP

#include <cstddef>
#include <cstdint>

namespace rpvg_cover {

// ---- the workgroup route (minPathCoverKernel) ------------------------------------------------------------------
constexpr uint32_t kWorkgroupMaxPaths = 9600;   // two vectors of doubles per path in 150 KiB of LDS

// ---- the grid route ------------------------------------------------------------------------------------------
// rows and entries of one cluster below 2^31: the library sorts count their items in `int`
constexpr uint64_t kGridMaxRows = 0x7fffffffull;
constexpr uint64_t kGridMaxEntries = 0x7fffffffull;
// A round is two launches (pick, strike); the host queues kChunkRounds of them, copies the control record behind them and looks
// at the copy of the chunk before: the last round of a cover falls anywhere between two looks.
constexpr uint32_t kChunkRounds = 32;
// pickKernel: a workgroup of kPickBlock threads takes a tile of kPickBlock * kPickPerThread consecutive paths, thread t the
// paths t, t + kPickBlock, ... of the tile; at most kPickMaxBlocks workgroups (beyond kPickMaxBlocks tiles a workgroup takes
// tiles b, b + kPickMaxBlocks, ...) — the pairs every workgroup of strikeKernel reduces
constexpr uint32_t kPickBlock = 256;
constexpr uint32_t kPickPerThread = 4;
constexpr uint32_t kPickTile = kPickBlock * kPickPerThread;
constexpr uint32_t kPickMaxBlocks = 256;
// strikeKernel: workgroups of kStrikeBlock threads over the chosen column, at most kStrikeMaxBlocks; a cluster of at most
// kHistPaths paths collects the struck gains in an LDS histogram per workgroup (64-bit bins: 16 KiB)
constexpr uint32_t kStrikeBlock = 256;
constexpr uint32_t kStrikeMaxBlocks = 1024;
constexpr uint32_t kHistPaths = 2048;

// ---- the route rule ----------------------------------------------------------------------------------------------
// Work is rows + entries of the cluster, as em_plan.hpp counts it.  The grid_min_work argument of rpvg_hip_min_path_cover_any:
//   0           the library default (kDefaultGridMinWork)
//   1           every cluster of at least two paths takes the grid route
//   UINT64_MAX  every cluster that fits the workgroup route stays on it ("width only")
//
// THE DEFAULT IS 2^16, MEASURED (profiles/path_cover_grid/ab.txt; tools/path_cover_grid_ab.py).  The rule: the smallest power of
// two of work from which ONE cluster alone is at least twice as fast on the grid route for EVERY measured cover length — twice,
// because the workgroup route takes a call's clusters side by side and the grid takes them one after the other.  MI355X, one
// cluster per call, 3 entries per row, wall time of the call; workgroup ms / grid ms, the smallest ratio over the widths
// (600 and 9 600 paths) for covers of about 8 | 100 | 500 or 1 000 paths:
//     work 2^10 (256 rows)      0.17 | 0.23 | 0.24      the grid loses: a round is two launches, and the host queues two chunks
//     work 2^12                 0.27 | 0.43 | 0.47      of kChunkRounds rounds before its first look (0.45 ms at the least)
//     work 2^14                 0.68 | 1.26 | 1.83
//     work 2^16 (16 384 rows)   2.39 | 5.21 | 6.83      <- the first size with the factor for every cover length
//     work 2^18                 5.26 | 15.6 | 25.7
//     work 2^20                 8.46 | 47.5 | 128
//     work 2^22 (2^20 rows)     9.15 | 62.1 | 337       (8.3 s against 25 ms at 9 600 paths and a cover of 1 000)
// (The table was taken with the default still at "width only" and the grid route forced by grid_min_work = 1: its last line
// says so.)
// What the factor of two does NOT cover: a call with MANY clusters between 2^16 and ~2^18 work.  The workgroup route runs 256 of
// them side by side in the time of the slowest, the grid 0.5 to 10 ms each, one after the other (the design document says so).
constexpr uint64_t kWidthOnly = UINT64_MAX;
constexpr uint64_t kDefaultGridMinWork = 1ull << 16;

inline uint64_t gridMinWork(const uint64_t argument) { return argument == 0 ? kDefaultGridMinWork : argument; }

enum Route : int { kRouteWorkgroup = 0, kRouteGrid = 1 };

// (paths, rows, entries of a cluster; the call's grid_min_work argument) -> route.  64-bit sizes: differences of 64-bit offsets.
inline int routeOf(const uint64_t paths, const uint64_t rows, const uint64_t entries, const uint64_t grid_min_work_argument) {
    if (paths <= 1) return kRouteWorkgroup;   // the cover of one path is {0}: nothing to run over a GPU
    if (paths > kWorkgroupMaxPaths) return kRouteGrid;
    const uint64_t work = rows + entries < rows ? UINT64_MAX : rows + entries;   // (saturating)
    const uint64_t threshold = gridMinWork(grid_min_work_argument);
    return threshold != kWidthOnly && work >= threshold ? kRouteGrid : kRouteWorkgroup;
}

// whether the grid route takes a cluster of these sizes at all (beyond: RPVG_HIP_ERR_INVALID before anything is launched)
inline bool gridFits(const uint64_t rows, const uint64_t entries) { return rows <= kGridMaxRows && entries <= kGridMaxEntries; }

// bits that hold 0 .. paths - 1 (at least one): the end bit of the sort by path
inline int sortBits(const uint64_t paths) {
    int bits = 1;
    while (bits < 64 && paths > 0 && ((paths - 1) >> bits)) ++bits;
    return bits;
}

// launches of a round
inline uint32_t pickBlocks(const uint64_t paths) {
    const uint64_t tiles = (paths + kPickTile - 1) / kPickTile;
    return static_cast<uint32_t>(tiles < 1 ? 1 : tiles > kPickMaxBlocks ? kPickMaxBlocks : tiles);
}
inline uint32_t strikeBlocks(const uint64_t rows) {   // (a column holds at most a cluster's rows — a malformed one more: the kernel strides)
    const uint64_t blocks = (rows + kStrikeBlock - 1) / kStrikeBlock;
    return static_cast<uint32_t>(blocks < 1 ? 1 : blocks > kStrikeMaxBlocks ? kStrikeMaxBlocks : blocks);
}
inline bool strikeUsesHistogram(const uint64_t paths) { return paths <= kHistPaths; }
// rounds the host queues at the most: a round chooses a path or finds nothing left
inline uint64_t maxRounds(const uint64_t paths) { return paths; }

// ---- the grid route's scratch, in elements ---------------------------------------------------------------------
struct GridScratch {
    uint64_t row_count;      // double   [rows]     the read count the cover sees (0 for a row whose noise is 1)
    uint64_t row_covered;    // uint32   [rows]
    uint64_t ent_row;        // uint32   [entries]  row of every entry, in row order
    uint64_t ent_index;      // uint32   [entries]  0, 1, 2, ...: the sort's values
    uint64_t sorted_path;    // uint32   [entries]  paths in column order
    uint64_t sorted_index;   // uint32   [entries]
    uint64_t col_row;        // uint32   [entries]  rows in column order
    uint64_t col_term;       // double   [entries]  count * log(prob) in column order
    uint64_t col_off;        // uint32   [paths + 1]
    uint64_t weight;         // double   [paths]
    uint64_t gain;           // uint64   [paths]
    uint64_t chosen_words;   // uint32   [ceil(paths / 32)]
    uint64_t pick_pairs;     // (double, uint32) [kPickMaxBlocks]
    uint64_t bytes;          // all of them
};
inline GridScratch gridScratch(const uint64_t paths, const uint64_t rows, const uint64_t entries) {
    GridScratch s;
    s.row_count = rows;
    s.row_covered = rows;
    s.ent_row = s.ent_index = s.sorted_path = s.sorted_index = s.col_row = s.col_term = entries;
    s.col_off = paths + 1;
    s.weight = s.gain = paths;
    s.chosen_words = (paths + 31) / 32;
    s.pick_pairs = kPickMaxBlocks;
    s.bytes = 8 * s.row_count + 4 * s.row_covered + 4 * (s.ent_row + s.ent_index + s.sorted_path + s.sorted_index + s.col_row) + 8 * s.col_term +
              4 * s.col_off + 8 * s.weight + 8 * s.gain + 4 * s.chosen_words + 12 * s.pick_pairs;
    return s;
}

}  // namespace rpvg_cover

#endif

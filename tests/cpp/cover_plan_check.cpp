// The decisions of the minimum path cover (rpvg_amd/csrc/cover_plan.hpp) on the CPU: the route of a cluster either side of the
// workgroup route's width and of the work threshold, at the three special threshold values, at one path and at the 31-bit
// edges; the launches of a round and the scratch of the grid route.  Prints "ok".
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/cover_plan_check.cpp
#include "cover_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace rpvg_cover;

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

int main(int argc, char ** argv) {
    if (argc > 1) {  // "limits": the plan's numbers for the Python tests to compare with the library's
        std::printf("%u %u %llu %llu %llu %u %u %u %u %u %u\n", kWorkgroupMaxPaths, kChunkRounds, static_cast<unsigned long long>(kDefaultGridMinWork),
                    static_cast<unsigned long long>(kGridMaxRows), static_cast<unsigned long long>(kGridMaxEntries), kPickBlock, kPickPerThread,
                    kPickMaxBlocks, kStrikeBlock, kStrikeMaxBlocks, kHistPaths);
        return 0;
    }
    const uint64_t never = UINT64_MAX, T = 1ull << 18;
    // width: limit - 1, limit, limit + 1 paths, whatever the threshold says about the work
    REQUIRE(routeOf(kWorkgroupMaxPaths - 1, 10, 30, never) == kRouteWorkgroup);
    REQUIRE(routeOf(kWorkgroupMaxPaths, 10, 30, never) == kRouteWorkgroup);
    REQUIRE(routeOf(kWorkgroupMaxPaths + 1, 10, 30, never) == kRouteGrid);
    REQUIRE(routeOf(kWorkgroupMaxPaths + 1, 10, 30, T) == kRouteGrid);
    REQUIRE(routeOf(kWorkgroupMaxPaths + 1, 1, 0, never) == kRouteGrid);
    REQUIRE(routeOf(65537, 64, 100, 0) == kRouteGrid);
    // work = rows + entries: threshold - 1, threshold
    REQUIRE(routeOf(600, T / 4, T / 4 * 3 - 1, T) == kRouteWorkgroup);
    REQUIRE(routeOf(600, T / 4, T / 4 * 3, T) == kRouteGrid);
    REQUIRE(routeOf(600, T / 4, T / 4 * 3 + 1, T) == kRouteGrid);
    REQUIRE(routeOf(2, T - 1, 0, T) == kRouteWorkgroup);
    REQUIRE(routeOf(2, T, 0, T) == kRouteGrid);
    REQUIRE(routeOf(kWorkgroupMaxPaths, T, 0, T) == kRouteGrid);
    // the three special values: 0 the default, 1 everything of two paths and more, UINT64_MAX width only
    REQUIRE(gridMinWork(0) == kDefaultGridMinWork && gridMinWork(1) == 1 && gridMinWork(never) == never && gridMinWork(77) == 77);
    REQUIRE(routeOf(600, 100, 300, 0) == routeOf(600, 100, 300, kDefaultGridMinWork));
    if (kDefaultGridMinWork != kWidthOnly) {
        REQUIRE(routeOf(600, kDefaultGridMinWork - 1, 0, 0) == kRouteWorkgroup);
        REQUIRE(routeOf(600, kDefaultGridMinWork, 0, 0) == kRouteGrid);
    } else {
        REQUIRE(routeOf(600, kGridMaxRows, kGridMaxEntries, 0) == kRouteWorkgroup);
    }
    REQUIRE(routeOf(2, 1, 0, 1) == kRouteGrid);
    REQUIRE(routeOf(2, 1, 1, 1) == kRouteGrid);
    REQUIRE(routeOf(kWorkgroupMaxPaths, 1, 1, 1) == kRouteGrid);
    REQUIRE(routeOf(2, kGridMaxRows, kGridMaxEntries, never) == kRouteWorkgroup);
    REQUIRE(routeOf(kWorkgroupMaxPaths, never / 2, never / 2, never) == kRouteWorkgroup);
    REQUIRE(routeOf(kWorkgroupMaxPaths, never, never, never) == kRouteWorkgroup);   // (the sum saturates; width only is width only)
    REQUIRE(routeOf(kWorkgroupMaxPaths, never, 2, T) == kRouteGrid);                  // (saturated, not wrapped to 1)
    // one path: the cover is {0}, never the grid
    REQUIRE(routeOf(1, 1, 1, 1) == kRouteWorkgroup);
    REQUIRE(routeOf(1, T, T, T) == kRouteWorkgroup);
    REQUIRE(routeOf(1, kGridMaxRows + 1, 0, 1) == kRouteWorkgroup);
    REQUIRE(routeOf(0, 1, 1, 1) == kRouteWorkgroup);   // (refused by the validation: an empty cluster)
    // the 31-bit edges of the grid route
    REQUIRE(gridFits(1, 0) && gridFits(kGridMaxRows, kGridMaxEntries));
    REQUIRE(gridFits(0x7fffffffull, 0x7fffffffull));
    REQUIRE(!gridFits(0x80000000ull, 1) && !gridFits(1, 0x80000000ull));
    REQUIRE(!gridFits(0x100000000ull, 0) && !gridFits(0, 0x100000001ull));   // would fit in 32 bits truncated
    // the sort's end bit
    REQUIRE(sortBits(0) == 1 && sortBits(1) == 1 && sortBits(2) == 1 && sortBits(3) == 2 && sortBits(4) == 2 && sortBits(5) == 3);
    REQUIRE(sortBits(kWorkgroupMaxPaths + 1) == 14 && sortBits(65536) == 16 && sortBits(65537) == 17 && sortBits(0xffffffffull) == 32);
    // a round's launches
    REQUIRE(pickBlocks(1) == 1 && pickBlocks(kPickTile) == 1 && pickBlocks(kPickTile + 1) == 2);
    REQUIRE(pickBlocks(static_cast<uint64_t>(kPickTile) * kPickMaxBlocks) == kPickMaxBlocks);
    REQUIRE(pickBlocks(static_cast<uint64_t>(kPickTile) * kPickMaxBlocks + 1) == kPickMaxBlocks && pickBlocks(0xffffffffull) == kPickMaxBlocks);
    REQUIRE(kPickMaxBlocks <= kStrikeBlock);   // a thread of a strike workgroup per pair
    REQUIRE(strikeBlocks(1) == 1 && strikeBlocks(kStrikeBlock) == 1 && strikeBlocks(kStrikeBlock + 1) == 2 && strikeBlocks(kGridMaxRows) == kStrikeMaxBlocks);
    REQUIRE(strikeUsesHistogram(kHistPaths) && !strikeUsesHistogram(kHistPaths + 1));
    REQUIRE(8ull * kHistPaths <= 64 * 1024);
    REQUIRE(maxRounds(2) == 2 && maxRounds(65537) == 65537);
    REQUIRE(kChunkRounds >= 2);
    // the scratch
    const GridScratch s = gridScratch(33, 10, 30);
    REQUIRE(s.row_count == 10 && s.row_covered == 10 && s.ent_row == 30 && s.col_term == 30 && s.col_off == 34 && s.weight == 33 && s.gain == 33);
    REQUIRE(s.chosen_words == 2 && s.pick_pairs == kPickMaxBlocks);
    REQUIRE(s.bytes == 80 + 40 + 4 * 150 + 240 + 136 + 264 + 264 + 8 + 12ull * kPickMaxBlocks);
    const GridScratch big = gridScratch(0xffffffffull, kGridMaxRows, kGridMaxEntries);
    REQUIRE(big.chosen_words == (1ull << 27) && big.bytes > (1ull << 36) && big.bytes < (1ull << 38));
    std::printf("ok\n");
    return 0;
}

// The decisions of the Gibbs samples table (rpvg_amd/csrc/gibbs_table_plan.hpp) on the CPU: the route of a cluster either side of
// every limit, at 0 paths and 0 blocks and at the 32-bit edges, the pitch and the LDS arithmetic of the staged piece, the tiles of a
// block, the launch of the global route and the sizes one table takes.  Prints "ok".
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/gibbs_table_plan_check.cpp
#include "gibbs_table_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace rpvg_gibbs_table;

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

int main(int argc, char ** argv) {
    if (argc > 1) {  // "limits": the limits for the Python tests to compare with the library's
        std::printf("%u %u %u %u %zu\n", kResidentPaths, kResidentColumns, kSampleTile, kGlobalPaths, residentLdsBytes(kResidentColumns));
        return 0;
    }
    // paths: limit - 1, limit, limit + 1 with the columns inside the route
    REQUIRE(routeOf(kResidentPaths - 1, 2) == kRouteResident);
    REQUIRE(routeOf(kResidentPaths, 2) == kRouteResident);
    REQUIRE(routeOf(kResidentPaths + 1, 2) == kRouteGlobal);
    // columns: the same with the paths inside the route
    REQUIRE(routeOf(100, kResidentColumns - 1) == kRouteResident);
    REQUIRE(routeOf(100, kResidentColumns) == kRouteResident);
    REQUIRE(routeOf(100, kResidentColumns + 1) == kRouteGlobal);
    // both at their limits, one beyond
    REQUIRE(routeOf(kResidentPaths, kResidentColumns) == kRouteResident);
    REQUIRE(routeOf(kResidentPaths + 1, kResidentColumns) == kRouteGlobal);
    REQUIRE(routeOf(kResidentPaths, kResidentColumns + 1) == kRouteGlobal);
    REQUIRE(routeOf(kResidentPaths + 1, kResidentColumns + 1) == kRouteGlobal);
    // 0 paths, 0 blocks (0 columns): nothing to scatter, counted for the route the sizes give
    REQUIRE(routeOf(0, 0) == kRouteResident);
    REQUIRE(routeOf(5, 0) == kRouteResident);
    REQUIRE(routeOf(0, 5) == kRouteResident);   // (refused by the validation: an id needs a path)
    REQUIRE(routeOf(kResidentPaths + 1, 0) == kRouteGlobal);
    // the 32-bit edges: sizes are differences of 64-bit offsets and are compared as such
    REQUIRE(routeOf(0xffffffffull, 1) == kRouteGlobal);
    REQUIRE(routeOf(1, 0xffffffffull) == kRouteGlobal);
    REQUIRE(routeOf(0x100000000ull, 0) == kRouteGlobal);                       // would be 0 paths in 32 bits
    REQUIRE(routeOf(0x100000000ull + kResidentPaths, 1) == kRouteGlobal);
    REQUIRE(routeOf(1, 0x100000000ull + kResidentColumns) == kRouteGlobal);
    REQUIRE(routeOf(0x7fffffffull, 0x7fffffffull) == kRouteGlobal);
    // the staged piece: an odd pitch for every width, one row of slack at most, inside the budget with four workgroups on a compute unit
    for (uint32_t c = 0; c <= kResidentColumns + 1; ++c) {
        REQUIRE(stagedPitch(c) % 2 == 1 && stagedPitch(c) >= c && stagedPitch(c) <= c + 1);
        // the 32 lanes of a cycle of ds_read_b64, at a stride of one row, on 32 different pairs of the 64 banks
        bool hit[32] = {};
        for (uint32_t lane = 0; lane < 32; ++lane) {
            const uint32_t pair = (lane * stagedPitch(c)) % 32;
            REQUIRE(!hit[pair]);
            hit[pair] = true;
        }
    }
    REQUIRE(residentLdsBytes(kResidentColumns) == 8 * kSampleTile * (kResidentColumns + 1));
    REQUIRE(residentLdsBytes(kResidentColumns - 1) == 8 * kSampleTile * (kResidentColumns - 1));
    REQUIRE(4 * residentLdsBytes(kResidentColumns) <= kLdsPerComputeUnit && residentLdsBytes(kResidentColumns) <= kLdsStaticMax);
    // tiles: 0 samples, either side of a tile, the 32-bit edge
    REQUIRE(tilesOf(0) == 0 && tilesOf(1) == 1 && tilesOf(kSampleTile - 1) == 1 && tilesOf(kSampleTile) == 1 && tilesOf(kSampleTile + 1) == 2);
    REQUIRE(tilesOf(0x7fffffffull) == (0x7fffffffull + kSampleTile - 1) / kSampleTile);
    REQUIRE(tileSamples(0, 0) == 0 && tileSamples(1, 0) == 1 && tileSamples(kSampleTile, 0) == kSampleTile && tileSamples(kSampleTile, 1) == 0);
    REQUIRE(tileSamples(kSampleTile + 1, 0) == kSampleTile && tileSamples(kSampleTile + 1, 1) == 1 && tileSamples(kSampleTile + 1, 2) == 0);
    REQUIRE(tileSamples(0x7fffffffull, tilesOf(0x7fffffffull) - 1) == (0x7fffffffull - 1) % kSampleTile + 1);
    REQUIRE(tileSamples(0x100000000ull + 3, 0x100000000ull / kSampleTile) == 3);
    // the global route's launch: a segment per kGlobalPaths paths, at least one, capped
    REQUIRE(pathSegments(0) == 0 && pathSegments(1) == 1 && pathSegments(kGlobalPaths) == 1 && pathSegments(kGlobalPaths + 1) == 2);
    REQUIRE(globalGridY(0) == 1 && globalGridY(kGlobalPaths) == 1 && globalGridY(kGlobalPaths + 1) == 2);
    REQUIRE(globalGridY(static_cast<uint64_t>(kGridYMax) * kGlobalPaths) == kGridYMax && globalGridY(static_cast<uint64_t>(kGridYMax) * kGlobalPaths + 1) == kGridYMax);
    REQUIRE(globalGridY(0x7fffffffull) == kGridYMax);
    // one table
    REQUIRE(sizesFit(0, 0, 0, 1, 0, 0, 0) && sizesFit(kMaxItems, kMaxItems, kMaxItems, kMaxItems, kMaxItems, kMaxItems, kMaxAbundanceSamples));
    REQUIRE(!sizesFit(kMaxItems + 1, 0, 0, 1, 0, 0, 0) && !sizesFit(0, kMaxItems + 1, 0, 1, 0, 0, 0) && !sizesFit(0, 0, kMaxItems + 1, 1, 0, 0, 0));
    REQUIRE(!sizesFit(0, 0, 0, 0x80000000ull, 0, 0, 0) && !sizesFit(0, 0, 0, 1, kMaxItems + 1, 0, 0) && !sizesFit(0, 0, 0, 1, 0, kMaxItems + 1, 0));
    REQUIRE(!sizesFit(0, 0, 0, 1, 0, 0, kMaxAbundanceSamples + 1));
    REQUIRE(tableFits(0, 0) && tableFits(kMaxItems, 0) && tableFits(kMaxCells, 1) && !tableFits(kMaxCells + 1, 1));
    REQUIRE(tableFits(kMaxCells / 1000, 1000) && !tableFits(kMaxCells / 1000 + 1, 1000) && !tableFits(kMaxItems, kMaxItems));
    std::printf("ok\n");
    return 0;
}

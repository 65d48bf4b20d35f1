// The decisions of the estimates table (rpvg_amd/csrc/estimates_plan.hpp) on the CPU: the route of a cluster either side of every
// limit, at the empty sizes and at the 32-bit edges, and the LDS arithmetic behind the limits.  Prints "ok".
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/estimates_plan_check.cpp
#include "estimates_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace rpvg_estimates;

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

int main(int argc, char ** argv) {
    if (argc > 1) {  // "limits": the limits for the Python tests to compare with the library's
        std::printf("%u %u %u %u %zu %zu\n", kWavePaths, kWaveMembers, kLdsPaths, kLdsMembers, residentLdsBytes(kWavePaths, kWaveMembers, kWaveBlock),
                    residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock));
        return 0;
    }
    // paths: limit - 1, limit, limit + 1 with the members inside the route
    REQUIRE(routeOf(kWavePaths - 1, 1) == kRouteWave);
    REQUIRE(routeOf(kWavePaths, 1) == kRouteWave);
    REQUIRE(routeOf(kWavePaths + 1, 1) == kRouteLds);
    REQUIRE(routeOf(kLdsPaths - 1, 1) == kRouteLds);
    REQUIRE(routeOf(kLdsPaths, 1) == kRouteLds);
    REQUIRE(routeOf(kLdsPaths + 1, 1) == kRouteGlobal);
    // members: the same with the paths inside the route
    REQUIRE(routeOf(1, kWaveMembers - 1) == kRouteWave);
    REQUIRE(routeOf(1, kWaveMembers) == kRouteWave);
    REQUIRE(routeOf(1, kWaveMembers + 1) == kRouteLds);
    REQUIRE(routeOf(1, kLdsMembers - 1) == kRouteLds);
    REQUIRE(routeOf(1, kLdsMembers) == kRouteLds);
    REQUIRE(routeOf(1, kLdsMembers + 1) == kRouteGlobal);
    // both at their limits; one inside the wavefront route and the other beyond the workgroup route
    REQUIRE(routeOf(kWavePaths, kWaveMembers) == kRouteWave);
    REQUIRE(routeOf(kLdsPaths, kLdsMembers) == kRouteLds);
    REQUIRE(routeOf(kWavePaths, kLdsMembers + 1) == kRouteGlobal);
    REQUIRE(routeOf(kLdsPaths + 1, kWaveMembers) == kRouteGlobal);
    REQUIRE(routeOf(kWavePaths + 1, kWaveMembers + 1) == kRouteLds);
    // nothing to do is the wavefront's
    REQUIRE(routeOf(0, 0) == kRouteWave);
    REQUIRE(routeOf(0, 5) == kRouteWave);   // (refused by the validation: a member needs a path)
    REQUIRE(routeOf(5, 0) == kRouteWave);
    REQUIRE(routeOf(kLdsPaths + 1, 0) == kRouteGlobal);
    // the 32-bit edges: sizes are differences of 64-bit offsets and are compared as such
    REQUIRE(routeOf(0xffffffffull, 1) == kRouteGlobal);
    REQUIRE(routeOf(1, 0xffffffffull) == kRouteGlobal);
    REQUIRE(routeOf(0x100000000ull, 0) == kRouteGlobal);          // would be 0 paths in 32 bits
    REQUIRE(routeOf(0x100000000ull + kWavePaths, 1) == kRouteGlobal);
    REQUIRE(routeOf(1, 0x100000000ull + kWaveMembers) == kRouteGlobal);
    REQUIRE(routeOf(0x7fffffffull, 0x7fffffffull) == kRouteGlobal);
    // the LDS of the resident routes: a word per path, per member and per wavefront, inside the budgets
    REQUIRE(residentLdsBytes(kWavePaths, kWaveMembers, kWaveBlock) == 4 * (kWavePaths + kWaveMembers + 1));
    REQUIRE(residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock) == 4 * (kLdsPaths + kLdsMembers + 4));
    REQUIRE(residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock) <= kLdsRouteBudget);
    REQUIRE(3 * residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock) <= kLdsPerComputeUnit);
    REQUIRE(32 * residentLdsBytes(kWavePaths, kWaveMembers, kWaveBlock) <= kLdsPerComputeUnit);
    REQUIRE(kLdsRouteBudget <= kLdsStaticMax);
    // bits of the placement's ballots and of the sort
    REQUIRE(bitsFor(0) == 1 && bitsFor(1) == 1 && bitsFor(2) == 1 && bitsFor(3) == 2 && bitsFor(4) == 2 && bitsFor(5) == 3);
    REQUIRE(bitsFor(kWavePaths) == 6 && bitsFor(kWavePaths + 1) == 7 && bitsFor(kLdsPaths) == 12);
    REQUIRE(bitsFor(0x80000000ull) == 31 && bitsFor(0x80000001ull) == 32);
    std::printf("ok\n");
    return 0;
}

// The decisions of the estimates table (estimates_table.hip; interface include/rpvg_table.h) as pure computations on sizes: the
// route of a cluster from its numbers of paths and members, and the LDS arithmetic behind the limits of the two cluster-resident
// routes.  Plain C++17, no HIP types: a CPU test reaches every decision (tests/cpp/estimates_plan_check.cpp).  The route rule is also
// device code (describeKernel).  This is the only place that knows the rule and the budget.
#ifndef RPVG_ESTIMATES_PLAN_HPP
#define RPVG_ESTIMATES_PLAN_HPP

#include <cstddef>
#include <cstdint>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_estimates {

enum Route : int { kRouteWave = 0, kRouteLds = 1, kRouteGlobal = 2, kRoutes = 3 };  // RPVG_TABLE_ROUTE_*

constexpr int kWaveBlock = 64;   // threads of a workgroup of the wavefront route
constexpr int kLdsBlock = 256;   // ... of the workgroup route

// A resident cluster keeps in LDS one 32-bit word per path (the histogram of the counting sort, scanned into the ends of the
// paths' slot ranges), one per member (the member positions in slot order) and one per wavefront (the scan's scratch).
constexpr RPVG_PLAN_FN size_t residentLdsBytes(const uint64_t paths, const uint64_t members, const int block) {
    return sizeof(uint32_t) * (static_cast<size_t>(paths) + static_cast<size_t>(members) + static_cast<size_t>(block) / 64);
}

// gfx950: 160 KiB of LDS per compute unit, 64 KiB of it at most for one workgroup's static allocation.  The workgroup route is
// to keep three workgroups (twelve wavefronts) on a compute unit, the wavefront route as many one-wave workgroups as the
// compute unit holds wavefronts (32): the budgets of a workgroup follow.
constexpr size_t kLdsPerComputeUnit = 160 * 1024;
constexpr size_t kLdsStaticMax = 64 * 1024;
constexpr size_t kLdsRouteBudget = kLdsPerComputeUnit / 3;    // 54 613 bytes
constexpr size_t kWaveRouteBudget = kLdsPerComputeUnit / 32;  // 5 120 bytes

constexpr uint32_t kWavePaths = 64, kWaveMembers = 256;   // the wavefront route
constexpr uint32_t kLdsPaths = 4096, kLdsMembers = 8192;  // the workgroup route: 48 KiB + 16 bytes

static_assert(residentLdsBytes(kWavePaths, kWaveMembers, kWaveBlock) <= kWaveRouteBudget, "wavefront route: LDS");
static_assert(residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock) <= kLdsRouteBudget, "workgroup route: LDS");
static_assert(kLdsRouteBudget <= kLdsStaticMax, "a static allocation");
static_assert(kWavePaths <= kLdsPaths && kWaveMembers <= kLdsMembers, "the routes nest");

// (paths, members) -> route.  64-bit arguments: the sizes are differences of 64-bit offsets.
RPVG_PLAN_FN int routeOf(const uint64_t paths, const uint64_t members) {
    if (paths <= kWavePaths && members <= kWaveMembers) return kRouteWave;
    if (paths <= kLdsPaths && members <= kLdsMembers) return kRouteLds;
    return kRouteGlobal;
}

// bits that hold 0 .. values - 1 (at least one): the ballots of the placement, the end bit of the sort
RPVG_PLAN_FN int bitsFor(const uint64_t values) {
    int bits = 1;
    while (bits < 64 && values > 0 && ((values - 1) >> bits)) ++bits;
    return bits;
}

}  // namespace rpvg_estimates

#endif

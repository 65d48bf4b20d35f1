// The decisions of the Gibbs samples table (gibbs_table.hip; interface include/rpvg_samples.h) as pure computations on sizes: the
// route of a cluster from its number of paths and the columns of its widest block, the pitch and the LDS arithmetic of the staged
// piece of the resident route, the tiles of a block and the items of the global route.  Plain C++17, no HIP types: a CPU test
// reaches every decision (tests/cpp/gibbs_table_plan_check.cpp).  The route rule and the pitch are also device code.  This is the
// only place that knows the rules and the budget.
#ifndef RPVG_GIBBS_TABLE_PLAN_HPP
#define RPVG_GIBBS_TABLE_PLAN_HPP

#include <cstddef>
#include <cstdint>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_gibbs_table {

enum Route : int { kRouteResident = 0, kRouteGlobal = 1, kRoutes = 2 };  // RPVG_GIBBS_ROUTE_*

constexpr int kBlock = 256;             // threads of a workgroup of every kernel: four wavefronts
constexpr uint32_t kSampleTile = 64;    // TS, the samples of a work item: a wavefront stores TS consecutive doubles of a row
constexpr uint32_t kResidentColumns = 64;   // a resident block's ids sit one in a lane of a wavefront
constexpr uint32_t kResidentPaths = 1024;   // ... and its items walk all paths of the cluster: 512 KiB of rows per item at most
constexpr uint32_t kGlobalPaths = 64 * (kBlock / 64);  // paths of a workgroup's item on the global route: 64 per wavefront

// The staged piece of the resident route: TS rows of `columns` doubles, sample-major as in the source.  The lanes of a wavefront
// read it along the samples, at a stride of one row: ds_read_b64 serves 32 lanes per cycle over 64 banks of 4 bytes, so a row of
// an even number of doubles puts lanes on the same banks.  The pitch is the next odd number: the 32 lanes of a cycle then hit the
// 32 even bank pairs once each.
constexpr RPVG_PLAN_FN uint32_t stagedPitch(const uint32_t columns) { return columns | 1u; }
constexpr RPVG_PLAN_FN size_t residentLdsBytes(const uint32_t columns) {
    return sizeof(double) * static_cast<size_t>(kSampleTile) * stagedPitch(columns);
}

// gfx950: 160 KiB of LDS per compute unit, 64 KiB of it at most for one workgroup's static allocation.  The resident route is to
// keep four workgroups (sixteen wavefronts) on a compute unit: the stores of one hide the staging of the next.
constexpr size_t kLdsPerComputeUnit = 160 * 1024;
constexpr size_t kLdsStaticMax = 64 * 1024;
constexpr size_t kResidentBudget = kLdsPerComputeUnit / 4;  // 40 960 bytes

static_assert(residentLdsBytes(kResidentColumns) <= kResidentBudget, "resident route: LDS");   // 64 * 65 * 8 = 33 280 bytes
static_assert(kResidentBudget <= kLdsStaticMax, "a static allocation");
static_assert(stagedPitch(kResidentColumns) % 2 == 1 && stagedPitch(kResidentColumns - 1) % 2 == 1, "odd pitch");
static_assert(kResidentColumns <= 64, "one id per lane");
static_assert(kSampleTile == 64, "one sample per lane");

// (paths of the cluster, columns of its widest block) -> route.  64-bit arguments: the sizes are differences of 64-bit offsets.
// A cluster without blocks (0 columns) or without paths has nothing to scatter; it counts for the route its sizes give.
RPVG_PLAN_FN int routeOf(const uint64_t paths, const uint64_t max_columns) {
    return (paths <= kResidentPaths && max_columns <= kResidentColumns) ? kRouteResident : kRouteGlobal;
}

// the sample tiles of a block of n samples, and the samples of tile t
RPVG_PLAN_FN uint64_t tilesOf(const uint64_t n) { return (n + kSampleTile - 1) / kSampleTile; }
RPVG_PLAN_FN uint32_t tileSamples(const uint64_t n, const uint64_t t) {
    const uint64_t begin = t * kSampleTile;
    if (begin >= n) return 0;
    return static_cast<uint32_t>(n - begin < kSampleTile ? n - begin : kSampleTile);
}

// the global route: a workgroup per (block, segment of kGlobalPaths paths); the second dimension of its launch for the widest
// cluster of the route, capped at what a grid takes (a workgroup then walks several segments)
constexpr uint32_t kGridYMax = 65535;
RPVG_PLAN_FN uint64_t pathSegments(const uint64_t paths) { return (paths + kGlobalPaths - 1) / kGlobalPaths; }
RPVG_PLAN_FN uint32_t globalGridY(const uint64_t max_paths) {
    const uint64_t segments = pathSegments(max_paths);
    return static_cast<uint32_t>(segments < 1 ? 1 : (segments > kGridYMax ? kGridYMax : segments));
}

// what one table takes: every count below 2^31 (32-bit words on the device), the abundance samples below 2^40
constexpr uint64_t kMaxItems = 0x7fffffffull;
constexpr uint64_t kMaxAbundanceSamples = 1ull << 40;
RPVG_PLAN_FN bool sizesFit(const uint64_t clusters, const uint64_t blocks, const uint64_t paths, const uint64_t gibbs_samples, const uint64_t path_ids,
                           const uint64_t noise_samples, const uint64_t abundance_samples) {
    return clusters <= kMaxItems && blocks <= kMaxItems && paths <= kMaxItems && gibbs_samples <= kMaxItems && path_ids <= kMaxItems &&
           noise_samples <= kMaxItems && abundance_samples <= kMaxAbundanceSamples;
}

// ... and its P x N cells below 2^36: half a terabyte of doubles, beyond any device, and far from a 64-bit overflow of the byte count
constexpr uint64_t kMaxCells = 1ull << 36;
RPVG_PLAN_FN bool tableFits(const uint64_t paths, const uint64_t gibbs_samples) {
    return gibbs_samples == 0 || paths <= kMaxCells / gibbs_samples;
}

}  // namespace rpvg_gibbs_table

#endif

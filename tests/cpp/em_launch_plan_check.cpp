// The merged EM launches of a solve's plan (rpvg_amd/csrc/em_plan.hpp, EmSolveKnobs::merged_launches) on the CPU: the tables for
// three and six side streams, with and without problems of more than 16 columns, with and without a problem too wide for LDS,
// the 256-thread launches (not merged: bin 2 on the main stream, bin 1 on a side stream) on both sides of 40 KB of streamed
// vectors, the roles of every launch with their grids; and that default-constructed knobs still give the tables
// of one launch per kernel variant.  Prints "ok".
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/em_launch_plan_check.cpp
#include "em_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rpvg_em;

#define REQUIRE(cond)                                                                            \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "%s:%d: case '%s': %s\n", __FILE__, __LINE__, g_case, #cond);   \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

static const char * g_case = "";

static EmSolveShape shapeOf(const uint32_t P, const uint32_t max_cols, const int side_streams) {
    EmSolveShape s;
    s.P = P;
    s.items_bound = P;
    s.max_cols = max_cols;
    s.max_cluster_paths = max_cols;
    s.max_cluster_work = 100;
    s.rows_capacity = 1000;
    s.cus = 256;
    s.side_streams = side_streams;
    s.hardware_queues = 4;
    return s;
}

static void requireTable(const EmSolvePlan & p, const std::vector<EmLaunch> & want) {
    REQUIRE(p.num_launches == static_cast<int>(want.size()));
    for (size_t i = 0; i < want.size(); ++i) {
        if (!(p.launches[i] == want[i])) {
            const EmLaunch & g = p.launches[i];
            std::fprintf(stderr, "launch %zu: bin %u variant %d grid %u lds %zu stream %d\n", i, g.bin, static_cast<int>(g.variant), g.grid, g.lds, g.stream);
        }
        REQUIRE(p.launches[i] == want[i]);
    }
}

// the roles of launch i: its bins in order, `grid` workgroups each — workgroup b of the launch is role b % variants, that bin's
// workgroup b / variants, so every workgroup of the launch's grid is exactly one (role, workgroup below the role's grid)
static void requireRoles(const EmSolvePlan & p, const int i, const std::vector<uint32_t> & bins, const uint32_t grid) {
    const EmRoles r = emLaunchRoles(p, p.launches[i]);
    REQUIRE(r.variants == bins.size() && r.variants >= 1 && r.variants <= kEmMaxRoles && r.grid == grid);
    for (uint32_t v = 0; v < r.variants; ++v) REQUIRE(r.bin[v] == bins[v]);
    // (kRegisterBins keeps its grid per bin in the table: the launch multiplies)
    const uint32_t total = r.variants * r.grid;
    REQUIRE(p.launches[i].variant == EmVariant::kRegisterBins ? p.launches[i].grid == r.grid : p.launches[i].grid == total);
    REQUIRE((total - 1) / r.variants == r.grid - 1 && (total - 1) % r.variants == r.variants - 1);   // the last workgroup: the last role's last
}

int main() {
    const EmVariant R = EmVariant::kRegisterBins, S256 = EmVariant::kSparse256Streamed, S1024 = EmVariant::kSparse1024Streamed;
    const EmVariant L64 = EmVariant::kSparse64Resident, L256 = EmVariant::kSparse256Resident, L1024 = EmVariant::kSparse1024Resident;
    const EmVariant W64 = EmVariant::kWaveBins, M1024 = EmVariant::kSparse1024Bins;
    const int M = kEmMainStream;
    EmSolveKnobs merged;
    merged.merged_launches = true;

    // 100 000 problems on 256 CUs: 256 and 512 workgroups per bin; 40 columns: 1 648 and 5 584 bytes for the streamed kernels' vectors
    g_case = "merged, six side streams, 40 columns";
    EmSolvePlan p = planEmSolve(shapeOf(100000, 40, 6), merged);
    REQUIRE(p.with_32_columns && !p.wide_possible);
    requireTable(p, {{4, W64, 3072, 32784, 3}, {2, S256, 256, 1648, M}, {1, L256, 512, 40960, 5}, {7, M1024, 512, 155648, 4}});
    requireRoles(p, 0, {6, 4, 5, 8, 9, 0}, 512);
    requireRoles(p, 1, {2}, 256);
    requireRoles(p, 2, {1}, 512);
    requireRoles(p, 3, {7, 3}, 256);
    // every launch of a side stream has a side stream of its own; one launch on the main stream
    for (int i = 0; i < p.num_launches; ++i) {
        for (int j = 0; j < i; ++j) REQUIRE(p.launches[i].stream != p.launches[j].stream);
    }

    g_case = "merged, three side streams";
    p = planEmSolve(shapeOf(100000, 40, 3), merged);
    requireTable(p, {{4, W64, 3072, 32784, 0}, {2, S256, 256, 1648, M}, {1, L256, 512, 40960, 1}, {7, M1024, 512, 155648, 2}});
    for (int i = 0; i < p.num_launches; ++i) {
        for (int j = 0; j < i; ++j) REQUIRE(p.launches[i].stream != p.launches[j].stream);
    }
    g_case = "merged, five side streams: as three";
    requireTable(planEmSolve(shapeOf(100000, 40, 5), merged), {{4, W64, 3072, 32784, 0}, {2, S256, 256, 1648, M}, {1, L256, 512, 40960, 1}, {7, M1024, 512, 155648, 2}});

    g_case = "merged, at most 16 columns";
    p = planEmSolve(shapeOf(100000, 16, 3), merged);
    REQUIRE(!p.with_32_columns);
    requireTable(p, {{4, W64, 2048, 32784, 0}, {2, S256, 256, 688, M}, {1, L256, 512, 40960, 1}, {7, M1024, 512, 155648, 2}});
    requireRoles(p, 0, {6, 4, 5, 0}, 512);
    REQUIRE(planEmSolve(shapeOf(100000, 17, 3), merged).launches[0].grid == 3072);

    g_case = "merged, the streamed vectors of four wavefronts around 40 KB";
    // 40 C + 48 bytes, in sixteens: 1 022 columns are 40 928 bytes, 1 023 are 40 976 — bin 2 has its own launch on either side
    REQUIRE(emLdsBytes(1022, 0, 0, 256, false) == 40928 && emLdsBytes(1023, 0, 0, 256, false) == 40976);
    requireTable(planEmSolve(shapeOf(100000, 1022, 3), merged), {{4, W64, 3072, 32784, 0}, {2, S256, 256, 40928, M}, {1, L256, 512, 40960, 1}, {7, M1024, 512, 155648, 2}});
    requireTable(planEmSolve(shapeOf(100000, 1023, 3), merged), {{4, W64, 3072, 32784, 0}, {2, S256, 256, 40976, M}, {1, L256, 512, 40960, 1}, {7, M1024, 512, 155648, 2}});
    requireTable(planEmSolve(shapeOf(100000, 1023, 6), merged), {{4, W64, 3072, 32784, 3}, {2, S256, 256, 40976, M}, {1, L256, 512, 40960, 5}, {7, M1024, 512, 155648, 4}});

    g_case = "merged, a wide problem";
    p = planEmSolve(shapeOf(100000, 3992, 3), merged);
    REQUIRE(!p.wide_possible && p.num_launches == 4 && p.launches[3].grid == 512 && p.launches[3].lds == 159744);   // (the streamed vectors: 156 KB)
    p = planEmSolve(shapeOf(100000, 3993, 3), merged);
    REQUIRE(p.wide_possible);
    requireTable(p, {{4, W64, 3072, 32784, 0}, {2, S256, 256, 159744, M}, {1, L256, 512, 40960, 1}, {7, M1024, 768, 159744, 2}});
    requireRoles(p, 3, {7, 3, 10}, 256);
    requireTable(planEmSolve(shapeOf(100000, 3993, 6), merged), {{4, W64, 3072, 32784, 3}, {2, S256, 256, 159744, M}, {1, L256, 512, 40960, 5}, {7, M1024, 768, 159744, 4}});

    g_case = "merged, few problems";
    // fewer problems than workgroups: a grid per role is at most the problems
    p = planEmSolve(shapeOf(300, 40, 3), merged);
    requireTable(p, {{4, W64, 1800, 32784, 0}, {2, S256, 256, 1648, M}, {1, L256, 300, 40960, 1}, {7, M1024, 512, 155648, 2}});
    p = planEmSolve(shapeOf(1, 40, 3), merged);
    requireTable(p, {{4, W64, 6, 32784, 0}, {2, S256, 1, 1648, M}, {1, L256, 1, 40960, 1}, {7, M1024, 2, 155648, 2}});
    requireRoles(p, 0, {6, 4, 5, 8, 9, 0}, 1);
    requireRoles(p, 3, {7, 3}, 1);

    g_case = "default knobs: a launch per kernel variant";
    const EmSolveKnobs defaults;
    REQUIRE(!defaults.merged_launches && defaults.one_register_launch);
    p = planEmSolve(shapeOf(100000, 40, 6), defaults);
    requireTable(p, {{4, R, 512, 32784, 3}, {2, S256, 256, 1648, M}, {3, S1024, 256, 5584, 0}, {0, L64, 512, 8192, 1}, {1, L256, 512, 40960, 5},
                     {7, L1024, 256, 155648, 4}});
    requireRoles(p, 0, {6, 4, 5, 8, 9}, 512);
    requireRoles(p, 3, {0}, 512);
    requireTable(planEmSolve(shapeOf(100000, 40, 3), defaults), {{4, R, 512, 32784, 0}, {2, S256, 256, 1648, M}, {3, S1024, 256, 5584, 2}, {0, L64, 512, 8192, 1},
                                                                 {1, L256, 512, 40960, 1}, {7, L1024, 256, 155648, 0}});
    p = planEmSolve(shapeOf(100000, 16, 6), defaults);
    requireRoles(p, 0, {6, 4, 5}, 512);

    g_case = "a launch per register bin: the merge does not apply";
    EmSolveKnobs five = merged;
    five.one_register_launch = false;
    EmSolveKnobs five_separate;
    five_separate.one_register_launch = false;
    const EmSolvePlan a = planEmSolve(shapeOf(100000, 40, 6), five), b = planEmSolve(shapeOf(100000, 40, 6), five_separate);
    REQUIRE(a.num_launches == 10 && a.num_launches == b.num_launches);
    for (int i = 0; i < a.num_launches; ++i) REQUIRE(a.launches[i] == b.launches[i]);

    std::printf("ok\n");
    return 0;
}

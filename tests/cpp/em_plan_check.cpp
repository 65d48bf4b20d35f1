// The decisions of an EM solve (rpvg_amd/csrc/em_plan.hpp) on the CPU.
//   em_plan_check            the plan at the sizes where a decision flips, against expectations written out here; prints "ok"
//   em_plan_check shapes     reads shapes "C rows entries" from the standard input, a line "-" ends a call; prints for every shape
//                            "bin mid dense route slot1 slot5" (emBinOf, the mid-size predicate, emDenseRule, the bin inside its
//                            call after the mid-size move, the statistics slot with one and with five register launches) and "-"
//                            behind every call — tests/test_em_bin_cases.py compares them with the Python restatement of the rule
//   g++ -std=c++17 -O1 -Wall -I rpvg_amd/csrc tests/cpp/em_plan_check.cpp
#include "em_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Shape {
    uint32_t C, rows, entries;
};

static void printCall(const std::vector<Shape> & call) {
    const EmBinRule rule = EmSolveKnobs().rule;
    uint32_t mid = 0;
    for (const Shape & s : call) mid += emIsMidSize(static_cast<uint32_t>(emBinOf(rule, s.C, s.rows, s.entries)), emWorkBucket(s.rows, s.entries)) ? 1u : 0u;
    const bool moved = emMidGridMoves(emMidGridAllowed(rule.grid_min_work), mid);
    for (const Shape & s : call) {
        const int bin = emBinOf(rule, s.C, s.rows, s.entries);
        const uint32_t bucket = emWorkBucket(s.rows, s.entries);
        const int route = emRouteOf(bin, bucket, moved);
        std::printf("%d %d %d %d %d %d\n", bin, emIsMidSize(static_cast<uint32_t>(bin), bucket) ? 1 : 0, emDenseRule(s.C, s.rows, s.entries) ? 1 : 0, route,
                    emStatsSlot(route, true), emStatsSlot(route, false));
    }
    std::printf("-\n");
}

static int printShapes() {
    std::vector<Shape> call;
    char line[256];
    while (std::fgets(line, sizeof(line), stdin)) {
        if (line[0] == '-') {
            printCall(call);
            call.clear();
            continue;
        }
        Shape s;
        if (std::sscanf(line, "%u %u %u", &s.C, &s.rows, &s.entries) != 3) {
            std::fprintf(stderr, "em_plan_check: not a shape: %s", line);
            return 1;
        }
        call.push_back(s);
    }
    if (!call.empty()) printCall(call);
    return 0;
}

static EmSolveShape shapeOf(const uint32_t P, const uint32_t max_cols, const uint64_t max_cluster_work) {
    EmSolveShape s;
    s.P = P;
    s.items_bound = P;
    s.max_cols = max_cols;
    s.max_cluster_paths = max_cols;
    s.max_cluster_work = max_cluster_work;
    s.rows_capacity = 1000;
    s.cus = 256;
    s.side_streams = 6;
    s.hardware_queues = 8;
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

static void checkGates() {
    g_case = "grid gate";
    EmSolveKnobs knobs;   // grid from 2^18 rows + entries: the mid-size move is allowed, the look starts at 2^16 - 1
    REQUIRE(planEmSolve(shapeOf(10, 8, (1u << 16) - 2), knobs).mid_grid_allowed);
    REQUIRE(!planEmSolve(shapeOf(10, 8, (1u << 16) - 2), knobs).grid_possible);
    REQUIRE(planEmSolve(shapeOf(10, 8, (1u << 16) - 1), knobs).grid_possible);
    knobs.rule.grid_min_work = 1u << 16;   // no mid-size move at or below 2^16: the look starts at the threshold itself
    REQUIRE(!planEmSolve(shapeOf(10, 8, (1u << 16) - 1), knobs).mid_grid_allowed);
    REQUIRE(!planEmSolve(shapeOf(10, 8, (1u << 16) - 1), knobs).grid_possible);
    REQUIRE(planEmSolve(shapeOf(10, 8, 1u << 16), knobs).grid_possible);
    knobs.rule.grid_min_work = (1u << 16) + 1;
    REQUIRE(planEmSolve(shapeOf(10, 8, 1), knobs).mid_grid_allowed);
    knobs.rule.grid_min_work = 1000;
    REQUIRE(!planEmSolve(shapeOf(10, 8, 999), knobs).grid_possible);
    REQUIRE(planEmSolve(shapeOf(10, 8, 1000), knobs).grid_possible);
    knobs.rule.grid_min_work = 0;   // never
    REQUIRE(!planEmSolve(shapeOf(10, 8, ~0ull), knobs).grid_possible);
    REQUIRE(!planEmSolve(shapeOf(10, 8, ~0ull), knobs).mid_grid_allowed);

    g_case = "mid-size verdict";
    REQUIRE(!emMidGridMoves(true, 0) && emMidGridMoves(true, 1) && emMidGridMoves(true, 8) && !emMidGridMoves(true, 9) && !emMidGridMoves(false, 3));
    REQUIRE(emIsMidSize(3, 15) && !emIsMidSize(3, 16) && !emIsMidSize(2, 0));
    REQUIRE(emWorkBucket(32767, 32767) == 16 && emWorkBucket(32767, 32768) == 15);   // work + 1 = 2^16 - 1 | 2^16
    REQUIRE(emRouteOf(3, 15, true) == 11 && emRouteOf(3, 15, false) == 3 && emRouteOf(3, 16, true) == 3 && emRouteOf(7, 0, true) == 7);

    g_case = "fused look and collapse";
    knobs = EmSolveKnobs();
    EmSolveShape s = shapeOf(10, 8, 1u << 20);
    REQUIRE(planEmSolve(s, knobs).fused_look && !planEmSolve(s, knobs).collapse);
    s.collapse_wanted = true;
    REQUIRE(planEmSolve(s, knobs).collapse && !planEmSolve(s, knobs).fused_look && !planEmSolve(s, knobs).collapse_too_large);
    REQUIRE(planEmSolve(s, knobs).collapse_max_rows == 1000);   // min(max_cluster_work, rows_capacity)
    s.max_cluster_work = 999;
    REQUIRE(planEmSolve(s, knobs).collapse_max_rows == 999);
    s.rows_capacity = 0;
    REQUIRE(!planEmSolve(s, knobs).collapse);
    s.rows_capacity = 0x7fffffffull;
    REQUIRE(!planEmSolve(s, knobs).collapse_too_large);
    s.rows_capacity = 0x80000000ull;
    REQUIRE(planEmSolve(s, knobs).collapse_too_large);
    s.rows_capacity = 1000;
    s.P = (1u << 20) - 2;
    REQUIRE(!planEmSolve(s, knobs).collapse_too_large);
    s.P = (1u << 20) - 1;
    REQUIRE(planEmSolve(s, knobs).collapse_too_large);
    s.collapse_wanted = false;
    REQUIRE(!planEmSolve(s, knobs).collapse_too_large);
    s = shapeOf(10, 8, 1u << 20);
    s.collapse_wanted = true;
    knobs.no_collapse = true;
    REQUIRE(!planEmSolve(s, knobs).collapse && planEmSolve(s, knobs).fused_look);
    knobs.no_fused_dense = true;
    REQUIRE(!planEmSolve(s, knobs).fused_look);
    REQUIRE(!planEmSolve(shapeOf(10, 8, 100), EmSolveKnobs()).fused_look);   // no grid, no look
}

static void checkGrids() {
    g_case = "grids";
    const EmSolveKnobs knobs;
    auto grids = [&](const uint32_t P, uint32_t * one, uint32_t * two) {
        const EmSolvePlan p = planEmSolve(shapeOf(P, 8, 100), knobs);
        *two = p.launches[0].grid;   // the register bins: two workgroups per CU
        *one = p.launches[1].grid;   // <256,false>: one
    };
    uint32_t one, two;
    grids(255, &one, &two);
    REQUIRE(one == 255 && two == 255);
    grids(256, &one, &two);
    REQUIRE(one == 256 && two == 256);
    grids(257, &one, &two);
    REQUIRE(one == 256 && two == 257);
    grids(512, &one, &two);
    REQUIRE(one == 256 && two == 512);
    grids(513, &one, &two);
    REQUIRE(one == 256 && two == 512);
    EmSolveKnobs scaled;
    scaled.grid_scale = 0.001;   // at least one workgroup
    REQUIRE(planEmSolve(shapeOf(1000, 8, 100), scaled).launches[0].grid == 1);

    g_case = "fill";
    EmSolveShape s = shapeOf(10, 8, 100);
    s.items_bound = 2047;
    REQUIRE(planEmFill(s, knobs).fill_grid == 2047 && planEmFill(s, knobs).dense_grid == 1024);
    s.items_bound = 2049;
    REQUIRE(planEmFill(s, knobs).fill_grid == 2048 && planEmFill(s, knobs).dense_grid == 1024);
    s.items_bound = 1023;
    REQUIRE(planEmFill(s, knobs).dense_grid == 1023);
    s.max_cluster_paths = 13;   // the map's capacity: a multiple of 4, at most 16 384 paths
    REQUIRE(planEmFill(s, knobs).lds_map_paths == 16 && planEmFill(s, knobs).fill_lds == 64);
    s.max_cluster_paths = 16384;
    REQUIRE(planEmFill(s, knobs).lds_map_paths == 16384 && planEmFill(s, knobs).fill_lds == 65536 && !(planEmFill(s, knobs).fill_lds > kLdsOptIn));
    s.max_cluster_paths = 16385;
    REQUIRE(planEmFill(s, knobs).lds_map_paths == 16384);
    s.max_cluster_work = (1u << 18) - 1;   // the wavefront-per-row scratch: 20 KB behind the map, from 2^18 rows + entries
    REQUIRE(!planEmFill(s, knobs).long_row_scratch);
    s.max_cluster_work = 1u << 18;
    REQUIRE(planEmFill(s, knobs).long_row_scratch && planEmFill(s, knobs).fill_lds == 65536 + 20480 && planEmFill(s, knobs).fill_lds > kLdsOptIn);
    EmSolveKnobs thread_rows;
    thread_rows.fill_thread_rows = true;
    REQUIRE(!planEmFill(s, thread_rows).long_row_scratch);
    // the fused build: 8 KB of scratch and four images of the widest row behind the map — 64 KB at a leading dimension of 1 792
    REQUIRE(emFillDenseLdsBytes(0, 1792) == 65536 && !(emFillDenseLdsBytes(0, 1792) > kLdsOptIn));
    REQUIRE(emFillDenseLdsBytes(0, 1794) == 65600 && emFillDenseLdsBytes(0, 1794) > kLdsOptIn);
    REQUIRE(emFillDenseLdsBytes(16, 1790) == 65536 && emFillDenseLdsBytes(20, 1790) > kLdsOptIn);
}

static void checkTables() {
    const EmVariant R = EmVariant::kRegisterBins, S256 = EmVariant::kSparse256Streamed, S1024 = EmVariant::kSparse1024Streamed;
    const EmVariant L64 = EmVariant::kSparse64Resident, L256 = EmVariant::kSparse256Resident, L1024 = EmVariant::kSparse1024Resident, W = EmVariant::kSparseWide;
    const int M = kEmMainStream;
    EmSolveKnobs knobs;
    // 100 000 problems on 256 CUs: 256 and 512 workgroups; 40 columns: 1 648 and 5 584 bytes for the streamed kernels' vectors
    g_case = "one register launch, six side streams";
    EmSolvePlan p = planEmSolve(shapeOf(100000, 40, 100), knobs);
    REQUIRE(!p.wide_possible && p.with_32_columns);
    requireTable(p, {{4, R, 512, 32784, 3}, {2, S256, 256, 1648, M}, {3, S1024, 256, 5584, 0}, {0, L64, 512, 8192, 1}, {1, L256, 512, 40960, 5},
                     {7, L1024, 256, 155648, 4}});
    REQUIRE(!planEmSolve(shapeOf(100000, 16, 100), knobs).with_32_columns && planEmSolve(shapeOf(100000, 17, 100), knobs).with_32_columns);
    g_case = "one register launch, six side streams, a wide problem";
    REQUIRE(!planEmSolve(shapeOf(100000, 3992, 100), knobs).wide_possible && planEmSolve(shapeOf(100000, 3992, 100), knobs).num_launches == 6);
    p = planEmSolve(shapeOf(100000, 3993, 100), knobs);
    REQUIRE(p.wide_possible);
    requireTable(p, {{4, R, 512, 32784, 3}, {2, S256, 256, 159744, M}, {3, S1024, 256, 159744, 0}, {0, L64, 512, 8192, 1}, {1, L256, 512, 40960, 5},
                     {7, L1024, 256, 155648, 4}, {10, W, 256, 144, 2}});
    g_case = "one register launch, three side streams";
    EmSolveShape three = shapeOf(100000, 3993, 100);
    three.side_streams = 3;
    requireTable(planEmSolve(three, knobs), {{4, R, 512, 32784, 0}, {2, S256, 256, 159744, M}, {3, S1024, 256, 159744, 2}, {0, L64, 512, 8192, 1},
                                             {1, L256, 512, 40960, 1}, {7, L1024, 256, 155648, 0}, {10, W, 256, 144, 2}});
    three.side_streams = 5;   // fewer than six: shared streams
    REQUIRE(planEmSolve(three, knobs).launches[0].stream == 0);

    knobs.one_register_launch = false;
    const EmVariant R1 = EmVariant::kRegister1x16, R2 = EmVariant::kRegister2x16, R4 = EmVariant::kRegister4x16, R1w = EmVariant::kRegister1x32, R2w = EmVariant::kRegister2x32;
    g_case = "five register launches, eight hardware queues";
    requireTable(planEmSolve(shapeOf(100000, 3993, 100), knobs),
                 {{6, R4, 512, 32784, 3}, {4, R1, 512, 8208, 4}, {5, R2, 512, 16400, 5}, {2, S256, 256, 159744, M}, {3, S1024, 256, 159744, 0},
                  {7, L1024, 256, 155648, 0}, {0, L64, 512, 8192, 1}, {1, L256, 512, 40960, 2}, {8, R1w, 256, 16400, 2}, {9, R2w, 256, 32784, 2},
                  {10, W, 256, 144, 5}});
    g_case = "five register launches, four hardware queues, narrow problems";
    EmSolveShape few = shapeOf(100000, 16, 100);
    few.hardware_queues = 7;
    requireTable(planEmSolve(few, knobs), {{6, R4, 512, 32784, 0}, {4, R1, 512, 8208, 1}, {5, R2, 512, 16400, 2}, {2, S256, 256, 688, M}, {3, S1024, 256, 2320, 0},
                                           {7, L1024, 256, 155648, 0}, {0, L64, 512, 8192, 1}, {1, L256, 512, 40960, 2}});
    few.hardware_queues = 8;
    knobs.few_streams = true;
    REQUIRE(planEmSolve(few, knobs).launches[0].stream == 0);
    knobs.few_streams = false;
    REQUIRE(planEmSolve(few, knobs).launches[0].stream == 3);

    g_case = "statistics slots";
    for (int b = 0; b < kEmBins; ++b) {
        const bool reg = b == 4 || b == 5 || b == 6 || b == 8 || b == 9;
        REQUIRE(emStatsSlot(b, false) == b);
        REQUIRE(emStatsSlot(b, true) == (reg ? 4 : b));
    }
}

static void checkSamplerAndLayout() {
    g_case = "sampler route";
    // 16 C + 48 bytes against 160 KB: 10 237 columns fit
    REQUIRE(gibbsOneWorkgroupLds(10237) == 163840 && gibbsOneWorkgroupLds(10238) > kGibbsOneWorkgroupLdsLimit);
    REQUIRE(!gibbsTakesGrid(10237, 10, 10, 0) && gibbsTakesGrid(10238, 10, 10, 0));
    REQUIRE(!gibbsTakesGrid(10, 30000, 35535, 65536) && gibbsTakesGrid(10, 30000, 35536, 65536) && !gibbsTakesGrid(10, 4000000000u, 4000000000u, 0));
    REQUIRE(!gibbsGridPossible(10237, 65535, 65536) && gibbsGridPossible(10238, 1, 65536) && gibbsGridPossible(10, 65536, 65536) && !gibbsGridPossible(10, ~0ull, 0));

    g_case = "storage layout";
    const uint64_t rows[3] = {10, 0, 5}, entries[3] = {7, 3, 0};
    uint64_t row_base[3], ent_base[3], rows_total = 0, entries_total = 0;
    emStorageBases(rows, entries, 3, row_base, ent_base, &rows_total, &entries_total);
    REQUIRE(row_base[0] == 0 && row_base[1] == 10 && row_base[2] == 10 && ent_base[0] == 0 && ent_base[1] == 7 && ent_base[2] == 10);
    REQUIRE(rows_total == 15 && entries_total == 10);
    // 20 bytes per row, 12 per entry: 420 bytes
    REQUIRE(emStorageByBound(rows_total, entries_total, 420) && emStorageByBound(rows_total, entries_total, 421) && !emStorageByBound(rows_total, entries_total, 419));
    const uint32_t kept[2] = {4, 6};
    emStorageBases(kept, kept, 2, row_base, ent_base, &rows_total, &entries_total);
    REQUIRE(row_base[1] == 4 && ent_base[1] == 4 && rows_total == 10 && entries_total == 10);
}

int main(int argc, char ** argv) {
    if (argc > 1 && std::strcmp(argv[1], "shapes") == 0) return printShapes();
    checkGates();
    checkGrids();
    checkTables();
    checkSamplerAndLayout();
    std::printf("ok\n");
    return 0;
}

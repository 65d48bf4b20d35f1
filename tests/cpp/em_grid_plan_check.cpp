// The launch shapes of the whole-GPU EM (rpvg_amd/csrc/em_plan.hpp: planEmGridCsr, planEmDense) on the CPU: lanes per row on both
// sides of a mean row length of 6, 24 and 96, workgroups against rows, the caps per CU and the partial vectors' bytes, rows per
// workgroup with a remainder, the strides at C = 63 | 64 | 65 and 15 | 16 | 17, the chunk of queued iterations at both ends, the
// A/B knobs; the dense kernels' switches at C = 128 | 129, 256 | 257, 512 | 513, 1024 | 1025, 1536 | 1537 and 2048, their grids
// at the caps and below the reduce slices.  Without arguments: prints "ok".  With "shapes <cus>": reads lines of "C rows entries"
// and prints, per line, the dense rule and both plans (tests/test_em_grid_cases.py compares them with the Python restatement).
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/em_grid_plan_check.cpp
#include "em_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rpvg_em;

#define REQUIRE(cond)                                                                            \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "%s:%d: case '%s': %s\n", __FILE__, __LINE__, g_case, #cond);   \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

static const char * g_case = "";

static void requireCsr(const EmGridCsrPlan & p, const int lanes, const uint32_t grid, const uint32_t rows_per_block, const uint32_t partial_ld,
                       const uint32_t update_grid, const size_t lds, const uint32_t chunk_its) {
    if (!(p.lanes == lanes && p.grid == grid && p.rows_per_block == rows_per_block && p.partial_ld == partial_ld && p.update_grid == update_grid &&
          p.lds == lds && p.chunk_its == chunk_its)) {
        std::fprintf(stderr, "lanes %d grid %u rows_per_block %u partial_ld %u update_grid %u lds %zu chunk_its %u\n", p.lanes, p.grid, p.rows_per_block,
                     p.partial_ld, p.update_grid, p.lds, p.chunk_its);
    }
    REQUIRE(p.lanes == lanes && p.grid == grid && p.rows_per_block == rows_per_block && p.partial_ld == partial_ld);
    REQUIRE(p.update_grid == update_grid && p.lds == lds && p.chunk_its == chunk_its);
}

static void requireDense(const EmDensePlan & p, const bool wide, const int nchunk, const uint32_t grid, const uint32_t partial_ld, const uint32_t slices) {
    if (!(p.wide == wide && p.nchunk == nchunk && p.grid == grid && p.partial_ld == partial_ld && p.reduce_slices == slices && p.chunk_its == 8)) {
        std::fprintf(stderr, "wide %d nchunk %d grid %u partial_ld %u reduce_slices %u chunk_its %u\n", p.wide ? 1 : 0, p.nchunk, p.grid, p.partial_ld,
                     p.reduce_slices, p.chunk_its);
    }
    REQUIRE(p.wide == wide && p.nchunk == nchunk && p.grid == grid && p.partial_ld == partial_ld && p.reduce_slices == slices && p.chunk_its == 8);
}

static void checkCsr() {
    g_case = "lanes by the mean row length";
    REQUIRE(emGridRowLanes(1000, 5999) == 1 && emGridRowLanes(1000, 6000) == 4);
    REQUIRE(emGridRowLanes(500, 11999) == 4 && emGridRowLanes(500, 12000) == 16);
    REQUIRE(emGridRowLanes(300, 28799) == 16 && emGridRowLanes(300, 28800) == 64);
    REQUIRE(emGridRowLanes(0, 0) == 1 && emGridRowLanes(1, 0xffffffffu) == 64);

    g_case = "one workgroup up to 256 rows of a thread each, two from 257";
    requireCsr(planEmGridCsr(20, 1, 2, 256), 1, 1, 1, 64, 2, 800, 32);
    requireCsr(planEmGridCsr(20, 3, 6, 256), 1, 1, 3, 64, 2, 800, 32);
    requireCsr(planEmGridCsr(20, 255, 510, 256), 1, 1, 255, 64, 2, 800, 32);
    requireCsr(planEmGridCsr(20, 256, 512, 256), 1, 1, 256, 64, 2, 800, 32);
    requireCsr(planEmGridCsr(20, 257, 514, 256), 1, 2, 129, 64, 2, 800, 32);

    g_case = "rows per workgroup with a remainder, a last workgroup of one row";
    requireCsr(planEmGridCsr(100, 100, 3000, 256), 16, 7, 15, 128, 7, 4000, 32);    // 6 x 15 + 10
    requireCsr(planEmGridCsr(200, 65, 6500, 256), 64, 17, 4, 256, 13, 8000, 32);    // 16 x 4 + 1
    requireCsr(planEmGridCsr(2049, 201, 201 * 2048, 256), 64, 51, 4, 2112, 129, 81960, 32);

    g_case = "the partial vectors stay below the CSR's bytes: at least 16 workgroups, then csr_bytes / (16 C)";
    requireCsr(planEmGridCsr(800, 4500, 9000, 256), 1, 16, 282, 832, 50, 32000, 32);      // 198 000 B / 12 800 = 15 -> 16
    requireCsr(planEmGridCsr(3000, 400, 38400, 256), 64, 16, 25, 3008, 188, 120000, 32);
    requireCsr(planEmGridCsr(3600, 1200, 115200, 256), 64, 24, 50, 3648, 225, 144000, 32);  // 1 406 400 B / 57 600 = 24

    g_case = "the caps: 2 workgroups per CU under one lane, 4 otherwise";
    requireCsr(planEmGridCsr(9, 131372, 262744, 256), 1, 512, 257, 64, 1, 360, 32);
    requireCsr(planEmGridCsr(9, 131072, 262144, 256), 1, 512, 256, 64, 1, 360, 32);
    requireCsr(planEmGridCsr(200, 5117, 96 * 5117, 256), 64, 1024, 5, 256, 13, 8000, 32);
    requireCsr(planEmGridCsr(200, 5117, 96 * 5117, 304), 64, 1024, 5, 256, 13, 8000, 32);   // (1 216 allowed, 1 280 wanted: 5 rows each all the same)
    requireCsr(planEmGridCsr(200, 5117, 96 * 5117, 80), 64, 320, 16, 256, 13, 8000, 32);
    requireCsr(planEmGridCsr(33, 4091, 40910, 256), 4, 64, 64, 64, 3, 1320, 32);
    requireCsr(planEmGridCsr(33, 4091, 40910, 8), 4, 32, 128, 64, 3, 1320, 32);

    g_case = "strides: the partials' at C = 63 | 64 | 65, the update's workgroups at C = 15 | 16 | 17";
    REQUIRE(planEmGridCsr(63, 300, 600, 256).partial_ld == 64 && planEmGridCsr(64, 300, 600, 256).partial_ld == 64 && planEmGridCsr(65, 300, 600, 256).partial_ld == 128);
    REQUIRE(planEmGridCsr(15, 300, 600, 256).update_grid == 1 && planEmGridCsr(16, 300, 600, 256).update_grid == 1 && planEmGridCsr(17, 300, 600, 256).update_grid == 2);
    REQUIRE(planEmGridCsr(3993, 300, 600, 256).lds == emGridLdsBytes(3993) && emGridLdsBytes(3993) <= kEmLdsLimit);

    g_case = "the chunk of queued iterations: 4 to 32, half a millisecond of streaming";
    REQUIRE(planEmGridCsr(40, 1000, 3000, 256).chunk_its == 32);
    // csr_bytes = 12 entries + 20 rows; iteration_us = csr_bytes / 4e6 + 8; chunk = clamp(500 / iteration_us, 4, 32), truncated
    REQUIRE(planEmGridCsr(40, 1, 2541665, 256).chunk_its == 32);            // 30 500 000 B: 15.625 us -> 32.0
    REQUIRE(planEmGridCsr(40, 1, 2541666, 256).chunk_its == 31);            // 30 500 012 B -> 31.99999
    REQUIRE(planEmGridCsr(40, 1000000, 9000000, 256).chunk_its == 12);      // 128 MB: 40 us -> 12.5
    REQUIRE(planEmGridCsr(40, 4000000, 32333333, 256).chunk_its == 4);      // 468 MB: 125 us -> 4.0
    REQUIRE(planEmGridCsr(40, 4000000, 100000000, 256).chunk_its == 4);

    g_case = "the A/B knobs";
    EmGridCsrKnobs lanes16;
    lanes16.row_lanes = 16;
    requireCsr(planEmGridCsr(20, 257, 514, 256, lanes16), 16, 17, 16, 64, 2, 800, 32);     // 16 x 16 + 1
    EmGridCsrKnobs blocks3;
    blocks3.blocks = 3;
    requireCsr(planEmGridCsr(20, 257, 514, 256, blocks3), 1, 3, 86, 64, 2, 800, 32);
    blocks3.blocks = 1000;   // (never more workgroups than rows)
    requireCsr(planEmGridCsr(20, 257, 514, 256, blocks3), 1, 257, 1, 64, 2, 800, 32);
}

static void checkDense() {
    g_case = "narrow kernel: one chunk up to 128 columns, two up to 256";
    requireDense(planEmDense(2, 300, 256), false, 1, 75, 2, 0);
    requireDense(planEmDense(3, 300, 256), false, 1, 75, 4, 0);
    requireDense(planEmDense(127, 301, 256), false, 1, 76, 128, 0);
    requireDense(planEmDense(128, 301, 256), false, 1, 76, 128, 0);
    requireDense(planEmDense(129, 301, 256), false, 2, 76, 130, 0);
    requireDense(planEmDense(255, 601, 256), false, 2, 151, 256, 0);
    requireDense(planEmDense(256, 601, 256), false, 2, 151, 256, 0);
    g_case = "wide kernel from 257 columns: chunks of 512";
    requireDense(planEmDense(257, 601, 256), true, 1, 301, 512, 16);
    requireDense(planEmDense(511, 601, 256), true, 1, 301, 512, 16);
    requireDense(planEmDense(512, 601, 256), true, 1, 301, 512, 16);
    requireDense(planEmDense(513, 601, 256), true, 2, 301, 1024, 16);
    requireDense(planEmDense(1023, 10, 256), true, 2, 5, 1024, 16);
    requireDense(planEmDense(1024, 10, 256), true, 2, 5, 1024, 16);
    requireDense(planEmDense(1025, 10, 256), true, 3, 5, 1536, 16);
    requireDense(planEmDense(1535, 10, 256), true, 3, 5, 1536, 16);
    requireDense(planEmDense(1536, 10, 256), true, 3, 5, 1536, 16);
    requireDense(planEmDense(1537, 10, 256), true, 4, 5, 2048, 16);
    requireDense(planEmDense(2047, 10, 256), true, 4, 5, 2048, 16);
    requireDense(planEmDense(2048, 201, 256), true, 4, 101, 2048, 16);
    g_case = "only the narrow kernel's one and two chunks are ever launched: wide takes everything above 256 columns";
    for (uint32_t C = 2; C <= kEmDenseMaxCols; ++C) {
        const EmDensePlan p = planEmDense(C, 1000, 256);
        REQUIRE(p.wide == (C > 256));
        REQUIRE(p.wide ? (p.nchunk >= 1 && p.nchunk <= 4 && static_cast<uint32_t>(p.nchunk) * 512 >= C && p.partial_ld == static_cast<uint32_t>(p.nchunk) * 512)
                       : (p.nchunk >= 1 && p.nchunk <= 2 && static_cast<uint32_t>(p.nchunk) * 128 >= C && p.partial_ld >= C && p.partial_ld % 2 == 0));
    }
    g_case = "grids: a row, the caps (2 | 4 workgroups per CU of 4 | 2 rows a trip) - 1, + 0, + 1, a rank without rows";
    requireDense(planEmDense(256, 1, 256), false, 2, 1, 256, 0);
    requireDense(planEmDense(256, 5, 256), false, 2, 2, 256, 0);
    requireDense(planEmDense(256, 2044, 256), false, 2, 511, 256, 0);
    requireDense(planEmDense(256, 2047, 256), false, 2, 512, 256, 0);
    requireDense(planEmDense(256, 2048, 256), false, 2, 512, 256, 0);
    requireDense(planEmDense(256, 2049, 256), false, 2, 512, 256, 0);    // (a second trip for one wavefront)
    requireDense(planEmDense(257, 1, 256), true, 1, 1, 512, 16);
    requireDense(planEmDense(257, 3, 256), true, 1, 2, 512, 16);
    requireDense(planEmDense(257, 31, 256), true, 1, 16, 512, 16);        // (as many partials as reduce slices; fewer below)
    requireDense(planEmDense(257, 2046, 256), true, 1, 1023, 512, 16);
    requireDense(planEmDense(257, 2047, 256), true, 1, 1024, 512, 16);
    requireDense(planEmDense(257, 2048, 256), true, 1, 1024, 512, 16);
    requireDense(planEmDense(257, 2049, 256), true, 1, 1024, 512, 16);    // (a second trip for the first workgroup: one row, parity 1)
    requireDense(planEmDense(2048, 1000000, 256), true, 4, 1024, 2048, 16);
    requireDense(planEmDense(2048, 0, 256), true, 4, 1, 2048, 16);
    g_case = "the A/B knob: workgroups per CU";
    requireDense(planEmDense(2048, 1000000, 256, 2), true, 4, 512, 2048, 16);
    requireDense(planEmDense(100, 1000000, 256, 8), false, 1, 2048, 100, 0);
}

// The fill's wavefront-per-row path adds up a row's sum in another order than the thread-per-row path: which one a cluster takes must not
// depend on the other clusters of the call, or a problem's last bits would change with its company.
static void checkFillLongRows() {
    g_case = "the fill's long-row path: by the cluster's own size and mean row length";
    REQUIRE(emFillLongRows(true, 4096, (1u << 18) - 4096));            // 2^18 rows + entries, 63 entries per row
    REQUIRE(!emFillLongRows(true, 4096, (1u << 18) - 4097));           // one unit of work less
    REQUIRE(!emFillLongRows(true, 300, 28800));                        // long rows, small cluster: a thread per row whatever else the call holds
    REQUIRE(emFillLongRows(true, 10000, 320000) && !emFillLongRows(true, 10000, 319999));   // a mean of 32 entries per row
    REQUIRE(!emFillLongRows(false, 4096, 1u << 20));                   // (the launch carries no scratch: RPVG_HIP_FILL_THREAD_ROWS, or no large cluster)
    EmSolveShape s;
    s.cus = 256;
    s.items_bound = 10;
    s.max_cluster_work = (1ull << 18) - 1;
    REQUIRE(!planEmFill(s, EmSolveKnobs()).long_row_scratch);
    s.max_cluster_work = 1ull << 18;                                   // (a cluster that takes the path is in a launch that carries the scratch)
    REQUIRE(planEmFill(s, EmSolveKnobs()).long_row_scratch);
}

int main(int argc, char ** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "shapes") == 0) {
        const uint32_t cus = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
        unsigned long long C, rows, entries;
        while (std::scanf("%llu %llu %llu", &C, &rows, &entries) == 3) {
            const uint32_t c = static_cast<uint32_t>(C), r = static_cast<uint32_t>(rows), e = static_cast<uint32_t>(entries);
            const EmGridCsrPlan s = planEmGridCsr(c, r, e, cus);
            std::printf("%d csr %d %u %u %u %u %zu %u", emDenseRule(c, r, e) ? 1 : 0, s.lanes, s.grid, s.rows_per_block, s.partial_ld, s.update_grid, s.lds,
                        s.chunk_its);
            if (c <= kEmDenseMaxCols) {
                const EmDensePlan d = planEmDense(c, r, cus);
                std::printf(" dense %d %d %u %u %u %u", d.wide ? 1 : 0, d.nchunk, d.grid, d.partial_ld, d.reduce_slices, d.chunk_its);
            }
            std::printf("\n");
        }
        return 0;
    }
    checkCsr();
    checkDense();
    checkFillLongRows();
    std::printf("ok\n");
    return 0;
}

// The decisions of an EM solve (em_sparse.hip) and of the read-count sampler (gibbs_counts.hip) as pure computations on sizes:
// the size bin of a problem, the few mid-size problems that move to the grid, the statistics slot of a bin, the storage layout
// of a host-made problem list, the sampler's route, and the plan of a solve — which looks at the device happen, the fill's
// grids and LDS, and the ordered table of the EM launches with their streams.  Plain C++17, no HIP types, no getenv: a CPU test
// reaches every decision (tests/cpp/em_plan_check.cpp).  The size rule is also device code (fillOffsetsKernel, emOrderKernel).
#ifndef RPVG_EM_PLAN_HPP
#define RPVG_EM_PLAN_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_em {

// ---- size bins of the EM kernels -----------------------------------------------
// One kernel variant per bin (rpvg_hip_em_kernel_name); the bin of a problem follows from its columns (paths + noise),
// kept rows and kept entries alone, so the device decides it (fillOffsetsKernel) and the host repeats the decision for
// the statistics:
//   0  LDS-resident, one wave      CSR + vectors fit 8 KB
//   1  LDS-resident, four waves    fit 40 KB
//   2  streamed from L2, 4 waves
//   3  streamed from L2, 16 waves  (a few giant problems)
//   4-6 register-resident dense, one wave: at most 16 columns and 64 / 128 / 256 rows (emRegisterKernel)
//   7  LDS-resident, sixteen waves  CSR + vectors fit 152 KB (one workgroup per CU: the whole LDS)
//   8-9 register-resident dense, one wave: 17 to 32 columns and 64 / 128 rows
//   10 too many columns for LDS-resident vectors (C >= 3 993): vectors in global memory, 16 waves
//   11 the grid bin: rows + entries at or above EmBinRule::grid_min_work — not one workgroup but the whole GPU, one round
//      of launches per EM iteration, driven by the host (em_grid.hip); no kernel of em_sparse.hip serves it
constexpr int kEmBins = 12;          // RPVG_HIP_EM_KERNELS
constexpr int kEmGridBin = 11;
constexpr int kEmWideBin = 10;
constexpr int kEmWorkBuckets = 32;   // inside a bin the problems are ordered by floor(log2(rows + entries)), large first
// A FEW mid-size problems — streamed ones (bin 3) of 2^16 rows + entries and more, below the grid threshold — take the grid route
// too: one workgroup walks such a problem at ~30 us per EM iteration (20 000 rows x 3 entries: 33), the whole GPU at ~8, and a real
// cluster of that size runs hundreds to thousands of iterations.  Only a few, because the grid takes its problems a handful at
// a time where the one-workgroup kernels take them all side by side: emOrderKernel moves them when the solve has at most
// kEmMidGridMax of them (the histogram tells it), and leaves them where they are otherwise.
constexpr uint32_t kEmMidGridMax = 8;
constexpr uint32_t kEmMidGridLog2 = 16;  // (a bucket is floor(log2(work + 1)): work + 1 >= 2^16)
constexpr uint32_t kEmMidBuckets = kEmWorkBuckets - kEmMidGridLog2;  // buckets 0 .. kEmMidBuckets - 1 hold work + 1 >= 2^16
constexpr int kEmStreamedBin = 3;
constexpr size_t kEmLdsLimit = 156 * 1024;
constexpr size_t kLdsOptIn = 64 * 1024;   // dynamic LDS above this needs hipFuncAttributeMaxDynamicSharedMemorySize
constexpr uint32_t kRegColsMax = 32;  // the widest register-resident variant
// The register-resident bins in ONE launch: workgroup b serves bin kRegisterBins[b % variants] (emRegisterKernel)
constexpr uint32_t kRegisterBins[5] = {6, 4, 5, 8, 9};  // <4,16> <1,16> <2,16> <1,32> <2,32>: rpvg_hip_em_kernel_name
constexpr uint32_t kRegisterKernelIndex = 4;             // the launch's slot in rpvg_hip_kernel_stats::em_kernel
// Launches of equal workgroup size in ONE launch (EmSolveKnobs::merged_launches): the wave launch — the register bins and bin 0 —
// under kRegisterKernelIndex, and the 1 024-thread launch (bins 7, 3 and, if possible, 10) under its first bin's slot
constexpr uint32_t kWaveSparseBin = 0;
constexpr uint32_t kSparse1024Bins[3] = {7, 3, 10};      // <1024,true> <1024,false> <1024,false,WIDE>
constexpr size_t kSparse1024ResidentLds = 152 * 1024;    // what bin 7 holds (emBinOf)

// LDS bytes of a problem: the abundance vector, one accumulator vector PER WAVEFRONT of the workgroup (the M-step's sums have one
// order of additions: emSparseProblem) and scratch, plus its CSR when resident
RPVG_PLAN_FN size_t emLdsBytes(uint32_t cols, uint32_t rows, uint32_t entries, int block, bool resident) {
    size_t bytes = sizeof(double) * ((1 + static_cast<size_t>(block) / 64) * cols + block / 64 + 2);
    if (resident) bytes += static_cast<size_t>(rows) * 16 + static_cast<size_t>(entries) * 8 + (static_cast<size_t>(rows) + 1 + entries) * 4 + 8;
    return (bytes + 15) & ~static_cast<size_t>(15);
}

// the grid route's workgroups (em_grid.hip: four wavefronts): abundances + an accumulator vector per wavefront
RPVG_PLAN_FN size_t emGridLdsBytes(const uint32_t cols) { return sizeof(double) * 5 * static_cast<size_t>(cols); }

// the staging tile of a register-resident variant (64 RPL rows of COLS columns)
RPVG_PLAN_FN size_t emRegisterLdsBytes(const int rpl, const int cols) { return (64 * static_cast<size_t>(rpl) * cols + 2) * sizeof(double); }

struct EmBinRule {
    uint32_t use_register_kernel;   // RPVG_HIP_NO_REGISTER_EM=1 clears it
    uint64_t streamed_small_work;   // a streamed problem above this many rows + entries gets 1 024 threads instead of 256
    uint64_t grid_min_work;         // rows + entries from which a problem goes to the grid bin (0: never; emGridMinWork())
};

RPVG_PLAN_FN int emBinOf(const EmBinRule rule, const uint32_t C, const uint32_t rows, const uint32_t entries) {
    const uint64_t work = static_cast<uint64_t>(entries) + rows;
    // (the grid kernels keep the vectors in LDS: the few problems too wide for that stay in bin 10)
    if (rule.grid_min_work != 0 && work >= rule.grid_min_work && emGridLdsBytes(C) <= kEmLdsLimit) return kEmGridBin;
    if (rule.use_register_kernel && C <= 16 && rows <= 256) return rows <= 64 ? 4 : rows <= 128 ? 5 : 6;
    if (rule.use_register_kernel && C <= kRegColsMax && rows <= 128) return rows <= 64 ? 8 : 9;
    if (emLdsBytes(C, rows, entries, 64, true) <= 8 * 1024) return 0;
    if (emLdsBytes(C, rows, entries, 256, true) <= 40 * 1024) return 1;
    if (emLdsBytes(C, rows, entries, 1024, true) <= 152 * 1024) return 7;
    // streamed: sixteen wavefronts if their accumulator vectors fit LDS, four if those do (up to ~3 900 columns), else the vectors
    // in global memory
    if (emLdsBytes(C, 0, 0, 256, false) > kEmLdsLimit) return kEmWideBin;
    if (emLdsBytes(C, 0, 0, 1024, false) > kEmLdsLimit) return 2;
    return work <= rule.streamed_small_work ? 2 : 3;
}

RPVG_PLAN_FN uint32_t emWorkBucket(const uint32_t rows, const uint32_t entries) {
    // floor(log2(work + 1)), inverted: bucket 0 holds the largest problems
    uint64_t work = static_cast<uint64_t>(entries) + rows + 1;
    uint32_t lg = 0;
    while (work > 1 && lg < static_cast<uint32_t>(kEmWorkBuckets - 1)) {
        work >>= 1;
        ++lg;
    }
    return static_cast<uint32_t>(kEmWorkBuckets - 1) - lg;
}

// a mid-size problem: a candidate of the move to the grid
RPVG_PLAN_FN bool emIsMidSize(const uint32_t bin, const uint32_t bucket) { return bin == static_cast<uint32_t>(kEmStreamedBin) && bucket < kEmMidBuckets; }
// (the few mid-size problems that may take the grid route: only where the grid route exists at all)
RPVG_PLAN_FN bool emMidGridAllowed(const uint64_t grid_min_work) { return grid_min_work > (1ull << kEmMidGridLog2); }
// the verdict of a solve with `mid` mid-size problems: they move
RPVG_PLAN_FN bool emMidGridMoves(const bool allowed, const uint32_t mid) { return allowed && mid > 0 && mid <= kEmMidGridMax; }
// the bin a problem runs in, inside its call
RPVG_PLAN_FN int emRouteOf(const int bin, const uint32_t bucket, const bool moved) {
    return moved && emIsMidSize(static_cast<uint32_t>(bin), bucket) ? kEmGridBin : bin;
}

RPVG_PLAN_FN bool emIsRegisterBin(const int bin) { return bin == 4 || bin == 5 || bin == 6 || bin == 8 || bin == 9; }
// (the register-resident bins of one launch are one kernel of the statistics: their problems together, the slowest of all)
RPVG_PLAN_FN int emStatsSlot(const int bin, const bool one_register_launch) {
    return emIsRegisterBin(bin) && one_register_launch ? static_cast<int>(kRegisterKernelIndex) : bin;
}

// ---- the dense sub-route of the grid bin (em_grid.hip, em_dense.hip) ------------------------------------
constexpr int kEmMaxFusedDense = 4;
constexpr uint32_t kEmDenseMaxCols = 2048;   // em_dense.hip: a row in the registers of one workgroup
// the dense matrix is the smaller representation (8 B per cell against 12 B per entry + 20 B per row) and a row is narrow enough
RPVG_PLAN_FN bool emDenseRule(const uint32_t columns, const uint32_t rows, const uint32_t entries) {
    if (columns > kEmDenseMaxCols || columns < 2) return false;
    const uint64_t ld = (static_cast<uint64_t>(columns) + 1) & ~1ull;
    return 8ull * rows * ld <= 12ull * entries + 20ull * rows;
}

// ---- the launch shapes of the whole-GPU EM (em_grid.hip: runEmGridProblems; em_dense.hip: emDenseIterate) ----------------
// Which kernel variant runs, over how many workgroups, with which strides and how many queued iterations per look at the control
// word: numbers of the problem's sizes and the GPU's CUs alone.  Both hosts launch what these say (tests/cpp/em_grid_plan_check.cpp,
// tests/em_grid_cases.py restates them).
constexpr uint32_t kEmGridBlock = 256;          // emGridAccumKernel: four wavefronts
constexpr uint32_t kEmGridUnroll = 4;           // rows a row slot walks at a time
constexpr uint32_t kEmGridUpdateBlock = 1024;   // emGridUpdateKernel: kEmGridUpdateColumns columns x 64 slices of the partials
constexpr uint32_t kEmGridUpdateColumns = 16;
constexpr uint32_t kEmDenseChunkIts = 8;        // em_dense.hip: iterations queued between looks at the control word
constexpr uint32_t kEmDenseReduceSlices = 16;   // the wide kernel's partials meet in this many slices first

// lanes per row of emGridAccumKernel by the mean row length
inline int emGridRowLanes(const uint32_t rows, const uint32_t entries) {
    const double mean = static_cast<double>(entries) / std::max(1u, rows);
    return mean < 6.0 ? 1 : mean < 24.0 ? 4 : mean < 96.0 ? 16 : 64;
}

struct EmGridCsrKnobs {     // A/B knobs of an EXPERIMENTS=1 build; 0: the rule
    int row_lanes = 0;      // RPVG_HIP_EM_GRID_ROW_LANES: 1, 4, 16, 64
    uint64_t blocks = 0;    // RPVG_HIP_EM_GRID_BLOCKS
};
struct EmGridCsrPlan {
    int lanes = 1;                 // emGridAccumKernel<lanes, kEmGridUnroll>
    uint32_t grid = 0;             // workgroups = partial vectors
    uint32_t rows_per_block = 0;   // a workgroup's contiguous rows (the last workgroup: what is left)
    uint32_t partial_ld = 0;       // doubles between two partial vectors
    uint32_t update_grid = 0;      // workgroups of emGridUpdateKernel
    size_t lds = 0;                // dynamic LDS of the pass
    uint32_t chunk_its = 0;        // iterations queued per chunk (two chunks in flight)
};
inline EmGridCsrPlan planEmGridCsr(const uint32_t C, const uint32_t rows, const uint32_t entries, const uint32_t cus, const EmGridCsrKnobs & knobs = EmGridCsrKnobs()) {
    EmGridCsrPlan p;
    p.lanes = knobs.row_lanes != 0 ? knobs.row_lanes : emGridRowLanes(rows, entries);
    // workgroups: enough to fill the GPU, few enough that the partial vectors (written and read once per iteration,
    // 16 B per column and workgroup) stay below the CSR's own bytes
    const uint64_t csr_bytes = 12ull * entries + 20ull * rows;
    const uint64_t slots = static_cast<uint64_t>(kEmGridBlock) / static_cast<uint64_t>(p.lanes);
    uint64_t blocks = (static_cast<uint64_t>(rows) + slots - 1) / slots;
    blocks = std::min<uint64_t>(blocks, static_cast<uint64_t>(cus) * (p.lanes == 1 ? 2 : 4));
    blocks = std::min<uint64_t>(blocks, std::max<uint64_t>(16, csr_bytes / (16ull * C)));
    if (knobs.blocks != 0) blocks = knobs.blocks;
    blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, rows));
    p.rows_per_block = static_cast<uint32_t>((static_cast<uint64_t>(rows) + blocks - 1) / blocks);
    p.grid = (rows + p.rows_per_block - 1) / p.rows_per_block;
    p.partial_ld = (C + 63) & ~63u;
    p.update_grid = (C + kEmGridUpdateColumns - 1) / kEmGridUpdateColumns;
    p.lds = emGridLdsBytes(C);
    // Iterations in chunks, two chunks in flight: the control word of chunk k is looked at while chunk k + 1 runs.
    // A short problem's iteration is a few microseconds, a giant one's milliseconds: the chunk holds about half a
    // millisecond of the problem's streaming time at the HBM rate, 4 to 32 iterations.
    const double iteration_us = static_cast<double>(csr_bytes) / 4.0e6 + 8.0;
    p.chunk_its = static_cast<uint32_t>(std::min(32.0, std::max(4.0, 500.0 / iteration_us)));
    return p;
}

struct EmDensePlan {
    bool wide = false;            // emDenseAccumWideKernel (a row split over the workgroup's four wavefronts) from 257 columns
    int nchunk = 1;               // narrow: emDenseAccumKernel<nchunk>, 128 columns each; wide: emDenseAccumWideKernel<nchunk>, 512 columns each
    uint32_t grid = 0;            // workgroups = partial vectors
    uint32_t partial_ld = 0;
    uint32_t reduce_slices = 0;   // wide: emDenseReducePartialsKernel's slices; narrow: none, the update reads the partials itself
    uint32_t chunk_its = kEmDenseChunkIts;
};
// blocks_per_cu_knob: RPVG_HIP_DENSE_BLOCKS_PER_CU (A/B knob; 0: the rule)
inline EmDensePlan planEmDense(const uint32_t C, const uint64_t rows, const uint32_t cus, const uint32_t blocks_per_cu_knob = 0) {
    EmDensePlan p;
    p.wide = C > 256;
    // enough waves to cover HBM latency, few enough partial vectors to reduce cheaply
    const uint32_t blocks_per_cu = blocks_per_cu_knob != 0 ? blocks_per_cu_knob : (p.wide ? 4u : 2u);
    const uint64_t rows_per_trip = p.wide ? 2 : 4;   // wide: a workgroup takes two rows per trip; narrow: a row per wavefront
    p.grid = static_cast<uint32_t>(std::min<uint64_t>((rows + rows_per_trip - 1) / rows_per_trip, static_cast<uint64_t>(cus) * blocks_per_cu));
    p.grid = std::max<uint32_t>(p.grid, 1);
    p.nchunk = p.wide ? static_cast<int>((C + 511) / 512) : static_cast<int>((C + 127) / 128);
    p.partial_ld = p.wide ? ((C + 511) / 512) * 512 : ((C + 1) & ~1u);
    p.reduce_slices = p.wide ? kEmDenseReduceSlices : 0;
    return p;
}

// ---- the compaction (fillSegmentsKernel, fillDenseRowsKernel) --------------------------------------------
constexpr uint32_t kLdsMapPaths = 16384;
constexpr uint32_t kFillSegmentRows = 1024;
constexpr uint64_t kFillLongRowEntries = 32;   // mean entries per row from which a cluster's rows take a wavefront each
constexpr size_t kFillLongRowLds = kFillSegmentRows * (3 * sizeof(uint32_t) + sizeof(double));
constexpr size_t kFillDenseLds = kFillSegmentRows * 2 * sizeof(uint32_t);   // + an image of a row per wavefront
constexpr uint64_t kFillLongRowMinWork = 1ull << 18;
// Whether the rows of a cluster take a wavefront each in the fill (and may go straight into a dense matrix): by the cluster's OWN rows + entries
// and mean row length, in a launch that carries the scratch (EmFillPlan::long_row_scratch) — never by what else the call holds.  The two paths add
// up a row's sum in different orders, so the normalised rows differ in their last bits: a cluster must take the same path in any company
// (tests/test_hip_em_grid_edges.py: every case in one call, bit-equal to the case alone).
RPVG_PLAN_FN bool emFillLongRows(const bool scratch, const uint64_t rows, const uint64_t entries) {
    return scratch && rows + entries >= kFillLongRowMinWork && entries >= kFillLongRowEntries * rows;
}
// LDS of the fused build: the column map, the scratch, an image of the widest matrix row for each of the four wavefronts
RPVG_PLAN_FN size_t emFillDenseLdsBytes(const uint32_t lds_map_paths, const uint64_t widest_ld) {
    return lds_map_paths * sizeof(int32_t) + kFillDenseLds + 4 * static_cast<size_t>(widest_ld) * sizeof(double);
}

// ---- what the environment may change (em_sparse.hip reads it: emSolveKnobs; the plan never does) ---------
struct EmSolveKnobs {
    EmBinRule rule = {1u, 0, 1ull << 18};  // RPVG_HIP_NO_REGISTER_EM, RPVG_HIP_EM_STREAM_SMALL, RPVG_HIP_EM_GRID_MIN_WORK
    bool no_collapse = false;          // RPVG_HIP_NO_EM_COLLAPSE, RPVG_HIP_NO_COLLAPSE
    bool no_fused_dense = false;       // RPVG_HIP_NO_FUSED_DENSE
    bool register_copies = true;       // RPVG_HIP_EM_COPIES
    bool one_register_launch = true;   // RPVG_HIP_EM_REGISTER_LAUNCHES=5 clears it
    bool merged_launches = false;      // the 64-thread and the 1 024-thread bins in one launch each (with one_register_launch): the library sets it (emSolveKnobs),
                                       // RPVG_HIP_EM_SEPARATE_LAUNCHES=1 clears it
    bool fill_thread_rows = false;     // RPVG_HIP_FILL_THREAD_ROWS: never a wavefront per row in the fill
    double grid_scale = 1.0;           // RPVG_HIP_EM_GRID_SCALE
    bool few_streams = false;          // RPVG_HIP_EM_FEW_STREAMS
    bool launch_early = false;         // RPVG_HIP_EM_LAUNCH_EARLY
    bool wait_sort_only = false;       // RPVG_HIP_EM_WAIT_SORT_ONLY
    bool join_on_stream = false;       // RPVG_HIP_EM_JOIN_ON_STREAM
    bool collapse_debug = false;       // RPVG_HIP_EM_COLLAPSE_DEBUG
    bool has_bound_bytes = false;      // RPVG_HIP_EM_BOUND_BYTES
    uint64_t bound_bytes = 0;
};

// ---- storage layout of a host-made problem list (prepareHostProblems) -------------------------------------
// Storage by the bound (a problem keeps at most the rows and entries of its cluster: one kernel counts and fills) up to a budget;
// beyond it two passes, the first of which only counts, and the storage is exact.
RPVG_PLAN_FN bool emStorageByBound(const uint64_t rows_bound, const uint64_t entries_bound, const uint64_t budget) {
    return rows_bound * 20 + entries_bound * 12 <= budget;
}
// the bases: problem p starts where the problems before it end
template <typename Count>
inline void emStorageBases(const Count * rows, const Count * entries, const uint32_t P, uint64_t * row_base, uint64_t * ent_base, uint64_t * rows_total,
                           uint64_t * entries_total) {
    uint64_t r = 0, e = 0;
    for (uint32_t p = 0; p < P; ++p) {
        row_base[p] = r;
        ent_base[p] = e;
        r += rows[p];
        e += entries[p];
    }
    *rows_total = r;
    *entries_total = e;
}

// ---- the read-count sampler's route (gibbs_counts.hip) -----------------------------------------------------
// gibbsReadCountKernel's LDS: abundances, counts, scratch.  A problem too wide for it, or of grid_min_work kept rows + entries
// and more (0: never for its size), takes the whole GPU (gibbs_grid.hip).
constexpr size_t kGibbsOneWorkgroupLdsLimit = 160 * 1024;
RPVG_PLAN_FN size_t gibbsOneWorkgroupLds(const uint32_t columns) {
    return (sizeof(double) * (2 * static_cast<size_t>(columns) + 256 / 64 + 2) + 15) & ~static_cast<size_t>(15);
}
RPVG_PLAN_FN bool gibbsTakesGrid(const uint32_t columns, const uint32_t rows, const uint32_t entries, const uint64_t grid_min_work) {
    const bool too_wide = gibbsOneWorkgroupLds(columns) > kGibbsOneWorkgroupLdsLimit;
    const bool too_large = grid_min_work != 0 && static_cast<uint64_t>(rows) + entries >= grid_min_work;
    return too_wide || too_large;
}
// whether a call can have such a problem at all (only then the host looks at the counts)
RPVG_PLAN_FN bool gibbsGridPossible(const uint32_t max_cols, const uint64_t max_cluster_work, const uint64_t grid_min_work) {
    return gibbsOneWorkgroupLds(max_cols) > kGibbsOneWorkgroupLdsLimit || (grid_min_work != 0 && max_cluster_work >= grid_min_work);
}

// ---- the plan of a solve --------------------------------------------------------------------------------
struct EmSolveShape {   // EmProblemList, the device and the context, as numbers
    uint32_t P = 0, items_bound = 0, max_cols = 0, max_cluster_paths = 0;
    uint64_t max_cluster_work = 0, rows_capacity = 0;
    unsigned long long wide_capacity = 0;
    uint32_t cus = 0;
    int side_streams = 6;      // real side streams of the context (of kEmSideStreams)
    int hardware_queues = 4;
    bool collapse_wanted = false;   // collapse_precision > 0
};
constexpr int kEmSideStreams = 6;   // rpvg_hip_ctx::kAuxStreams
constexpr uint32_t kEmCollapseMaxProblems = (1u << 20) - 2;   // kCollapseMaxMatrices: the matrix field of the collapse's sort key
constexpr uint64_t kEmCollapseMaxRows = 0x7fffffffull;

// the compaction's launches: what the counting pass, the sampler and the solve share
struct EmFillPlan {
    uint32_t fill_grid = 0;       // fillSegmentsKernel<*>: a few workgroups per CU (an item is at most 1 024 rows)
    uint32_t dense_grid = 0;      // fillDenseRowsKernel, per fused problem
    uint32_t lds_map_paths = 0;   // capacity of the LDS column map (a multiple of 4)
    bool long_row_scratch = false;  // the launches carry kFillLongRowLds behind the map: clusters of long rows take a wavefront per row
    size_t fill_lds = 0;
};
inline EmFillPlan planEmFill(const EmSolveShape & s, const EmSolveKnobs & knobs) {
    EmFillPlan f;
    f.fill_grid = std::min<uint32_t>(s.items_bound, s.cus * 8);
    f.dense_grid = std::min<uint32_t>(s.items_bound, s.cus * 4);
    // (the scratch behind the map holds doubles, and fillDenseRowsKernel moves 16 bytes at a time)
    f.lds_map_paths = (std::min<uint32_t>(s.max_cluster_paths, kLdsMapPaths) + 3) & ~3u;
    // The wavefront-per-row path costs 20 KB of LDS per workgroup: only a solve that sits on a cluster large enough to matter
    // (the grid threshold of the EM: a batch of small clusters keeps its eight workgroups per CU) carries it.
    f.long_row_scratch = !knobs.fill_thread_rows && s.max_cluster_work >= kFillLongRowMinWork;
    f.fill_lds = f.lds_map_paths * sizeof(int32_t) + (f.long_row_scratch ? kFillLongRowLds : 0);
    return f;
}

enum class EmVariant : uint8_t {
    kSparse64Resident, kSparse256Resident, kSparse1024Resident, kSparse256Streamed, kSparse1024Streamed, kSparseWide,
    kRegisterBins,   // the register-resident bins in one launch (emRegisterKernel)
    kRegister1x16, kRegister2x16, kRegister4x16, kRegister1x32, kRegister2x32,   // one launch per bin (emRegisterBinKernel)
    // merged launches of one workgroup size (emRegisterKernel, emSparseRolesKernel): their roles are emLaunchRoles
    kWaveBins,         // the register-resident bins and bin 0
    kSparse1024Bins    // bins 7 and 3, and 10 if a problem can be that wide
};
constexpr int kEmMainStream = -1;
struct EmLaunch {
    uint32_t bin;        // the bin the launch serves (a merged launch: the first of its bins), and the slot of its span in the statistics
    EmVariant variant;
    uint32_t grid;       // workgroups of the persistent launch
    size_t lds;          // dynamic LDS bytes
    int stream;          // kEmMainStream, or side stream k of the context
};
inline bool operator==(const EmLaunch & a, const EmLaunch & b) {
    return a.bin == b.bin && a.variant == b.variant && a.grid == b.grid && a.lds == b.lds && a.stream == b.stream;
}
constexpr int kEmMaxLaunches = 11;

// The roles of a launch that serves several bins: workgroup b serves bin[b % variants] as that bin's workgroup b / variants — the roles
// side by side from the first workgroup on, `grid` workgroups each; a workgroup keeps its role for its lifetime (a launch of one bin:
// one role)
constexpr uint32_t kEmMaxRoles = 6;
struct EmRoles {
    uint32_t variants = 0;
    uint32_t grid = 0;   // workgroups per role: the launch has variants * grid
    uint32_t bin[kEmMaxRoles] = {};
};

struct EmSolvePlan {
    EmFillPlan fill;
    bool collapse = false;            // readCollapseProbabilityMatrix on the rows of every problem
    bool collapse_too_large = false;  // ... of a solve beyond what one collapse indexes: an error
    uint64_t collapse_max_rows = 0;   // a bound of the rows of the largest problem
    bool mid_grid_allowed = false;
    // The grid bin (problems too large for one workgroup, em_grid.hip): the host has to see them.  Only a solve that
    // sits on a cluster large enough to produce one pays for the look (two small copies and their waits).
    bool grid_possible = false;
    bool fused_look = false;          // the host looks for problems whose dense matrix the compaction writes itself
    bool wide_possible = false;       // a problem may be too wide for LDS-resident vectors (bin 10)
    bool with_32_columns = false;     // a problem may have more than 16 columns (bins 8 and 9)
    int num_launches = 0;
    EmLaunch launches[kEmMaxLaunches];
};

// Workgroups of a persistent launch: one or two per CU (or the bound on the problems if smaller) — every workgroup of a
// grid costs the dispatcher ~40 ns even if it finds its bin empty, and the host launches all variants blindly: grids
// sized by what the GPU could hold (4 096 waves for the register kernel) were 20 000 idle workgroups per call, 0.7 ms
// of dispatcher time next to the other lane's kernels.  A queue of 1 200 short problems drains through 512 waves in
// tens of microseconds; the problems that run for thousands of iterations start that much later at the most.
inline uint32_t emLaunchGrid(const EmSolveShape & s, const EmSolveKnobs & knobs, const uint32_t per_cu) {
    return std::min<uint32_t>(s.P, std::max<uint32_t>(1, static_cast<uint32_t>(s.cus * per_cu * knobs.grid_scale)));
}

// The bins are independent, so their tails (a small problem that needs thousands of iterations, a giant one with
// many rows) should overlap — but only as many kernels run side by side as the runtime has hardware queues.
// Default-constructed knobs: one persistent launch per kernel variant; chains of launches that share a stream run one after the
// other: balanced by the kernels' usual durations.  The register-resident bins in one launch, first — they are the long
// ones —, the others balanced over the side streams: with six side streams everybody has a stream of its own, with three (the contexts of the batch pipeline) the launch of
// the register bins (1.3 ms on the configs[2] batch) and <1024,true> (0.2) share one, <64,true> (0.9) and <256,true> (0.5)
// another, and <1024,false> (0.8) and the wide one have the third.
// RPVG_HIP_EM_REGISTER_LAUNCHES=5: a launch per register bin; with eight hardware queues the first three get streams of their own.
// EmSolveKnobs::merged_launches (what the library runs; RPVG_HIP_EM_SEPARATE_LAUNCHES=1 gives the table above): a chain of two
// launches lasts as long as both, and every launch holds a hardware queue that other batches' streams share, for as long as its
// slowest problem iterates.  Launches of equal workgroup size therefore share a launch, as the register bins do, and every launch
// of a side stream has a side stream of its own (0, 1, 2 with three side streams; 3, 5, 4 with six):
//   64 threads    the register bins and bin 0 (<64,true>), under the LDS of the largest staging tile
//   256 threads   bin 1 (<256,true>)
//   1 024 threads bins 7 (<1024,true>), 3 (<1024,false>) and, if possible, 10 (the wide one) under the largest of their LDS
// A workgroup's role is fixed by its index (EmRoles); the grid is the sum of the roles' grids, which are equal.  <256,false> (bin 2) stays a launch
// of its own on the main stream: with no launch there at all — bins 1 and 2 in one launch on a side stream — the configs[2]
// pipeline ran 0.2 ms per batch SLOWER than with this empty launch in place (profiles/em_launches/ab.txt), and a problem reaches
// bin 2 only from 1 174 columns on, where its vectors would not fit next to bin 1's 40 KB anyway.
inline EmSolvePlan planEmSolve(const EmSolveShape & s, const EmSolveKnobs & knobs) {
    EmSolvePlan p;
    p.fill = planEmFill(s, knobs);
    p.collapse = s.collapse_wanted && !knobs.no_collapse && s.rows_capacity > 0;
    // (the collapse indexes rows with 32 bits and matrices with 20; the callers' memory budgets keep a solve far below both)
    p.collapse_too_large = p.collapse && !(s.rows_capacity <= kEmCollapseMaxRows && s.P <= kEmCollapseMaxProblems);
    p.collapse_max_rows = std::min<uint64_t>(s.max_cluster_work, s.rows_capacity);  // (rows + entries of the largest cluster: a bound of its rows)
    const uint64_t grid_min_work = knobs.rule.grid_min_work;
    p.mid_grid_allowed = emMidGridAllowed(grid_min_work);
    p.grid_possible = grid_min_work != 0 && s.max_cluster_work >= (p.mid_grid_allowed ? (1ull << kEmMidGridLog2) - 1 : grid_min_work);
    // (a solve whose problems are collapsed keeps the CSR: row_collapse.hip reads it)
    p.fused_look = p.grid_possible && !p.collapse && !knobs.no_fused_dense;
    const size_t streamed_lds_256 = emLdsBytes(s.max_cols, 0, 0, 256, false), streamed_lds_1024 = emLdsBytes(s.max_cols, 0, 0, 1024, false);
    p.wide_possible = streamed_lds_256 > kEmLdsLimit;
    p.with_32_columns = s.max_cols > 16;

    const uint32_t g1 = emLaunchGrid(s, knobs, 1), g2 = emLaunchGrid(s, knobs, 2);
    const size_t lds_256 = std::min(streamed_lds_256, kEmLdsLimit), lds_1024 = std::min(streamed_lds_1024, kEmLdsLimit);
    const size_t lds_wide = sizeof(double) * (1024 / 64 + 2);
    auto add = [&p](const uint32_t bin, const EmVariant v, const uint32_t grid, const size_t lds, const int stream) {
        p.launches[p.num_launches++] = EmLaunch{bin, v, grid, lds, stream};
    };
    if (knobs.one_register_launch && knobs.merged_launches) {
        const bool own = s.side_streams >= kEmSideStreams;
        const uint32_t wave_roles = (p.with_32_columns ? 5u : 3u) + 1u;
        add(kRegisterKernelIndex, EmVariant::kWaveBins, g2 * wave_roles, emRegisterLdsBytes(4, 16), own ? 3 : 0);
        add(2, EmVariant::kSparse256Streamed, g1, lds_256, kEmMainStream);
        add(1, EmVariant::kSparse256Resident, g2, 40 * 1024, own ? 5 : 1);
        add(kSparse1024Bins[0], EmVariant::kSparse1024Bins, g1 * (p.wide_possible ? 3u : 2u), std::max(kSparse1024ResidentLds, std::max(lds_1024, lds_wide)),
            own ? 4 : 2);
        return p;
    }
    if (knobs.one_register_launch) {
        const bool own = s.side_streams >= kEmSideStreams;
        add(kRegisterKernelIndex, EmVariant::kRegisterBins, g2, emRegisterLdsBytes(4, 16), own ? 3 : 0);  // (the largest staging tile: 4 x 16 = 2 x 32)
        add(2, EmVariant::kSparse256Streamed, g1, lds_256, kEmMainStream);
        add(3, EmVariant::kSparse1024Streamed, g1, lds_1024, own ? 0 : 2);
        add(0, EmVariant::kSparse64Resident, g2, 8 * 1024, 1);
        add(1, EmVariant::kSparse256Resident, g2, 40 * 1024, own ? 5 : 1);
        add(7, EmVariant::kSparse1024Resident, g1, 152 * 1024, own ? 4 : 0);
        if (p.wide_possible) add(kEmWideBin, EmVariant::kSparseWide, g1, lds_wide, 2);
        return p;
    }
    const bool many_queues = s.hardware_queues >= 8 && !knobs.few_streams;
    const int s_reg4 = many_queues ? 3 : 0, s_reg1 = many_queues ? 4 : 1, s_reg2 = many_queues ? 5 : 2;
    add(6, EmVariant::kRegister4x16, g2, emRegisterLdsBytes(4, 16), s_reg4);
    add(4, EmVariant::kRegister1x16, g2, emRegisterLdsBytes(1, 16), s_reg1);
    add(5, EmVariant::kRegister2x16, g2, emRegisterLdsBytes(2, 16), s_reg2);
    add(2, EmVariant::kSparse256Streamed, g1, lds_256, kEmMainStream);
    add(3, EmVariant::kSparse1024Streamed, g1, lds_1024, 0);
    add(7, EmVariant::kSparse1024Resident, g1, 152 * 1024, 0);
    add(0, EmVariant::kSparse64Resident, g2, 8 * 1024, 1);
    add(1, EmVariant::kSparse256Resident, g2, 40 * 1024, 2);
    if (p.with_32_columns) {
        add(8, EmVariant::kRegister1x32, g1, emRegisterLdsBytes(1, 32), 2);
        add(9, EmVariant::kRegister2x32, g1, emRegisterLdsBytes(2, 32), 2);
    }
    if (p.wide_possible) add(kEmWideBin, EmVariant::kSparseWide, g1, lds_wide, s_reg2);
    return p;
}

// the roles of a row of the plan's table (a row of one bin: that bin with the row's grid)
inline EmRoles emLaunchRoles(const EmSolvePlan & p, const EmLaunch & l) {
    EmRoles r;
    const uint32_t register_bins = p.with_32_columns ? 5u : 3u;
    switch (l.variant) {
        case EmVariant::kRegisterBins:   // (its grid is the grid per bin)
        case EmVariant::kWaveBins:
            for (uint32_t v = 0; v < register_bins; ++v) r.bin[r.variants++] = kRegisterBins[v];
            if (l.variant == EmVariant::kWaveBins) r.bin[r.variants++] = kWaveSparseBin;
            break;
        case EmVariant::kSparse1024Bins:
            for (uint32_t v = 0; v < (p.wide_possible ? 3u : 2u); ++v) r.bin[r.variants++] = kSparse1024Bins[v];
            break;
        default: r.bin[r.variants++] = l.bin; break;
    }
    r.grid = l.variant == EmVariant::kRegisterBins ? l.grid : l.grid / r.variants;
    return r;
}

}  // namespace rpvg_em

#endif

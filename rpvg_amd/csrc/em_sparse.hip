// Batched EM abundance solves on ragged, sparse cluster problems (gfx950).
//
// Takes over, for a whole batch of (cluster, column-subset) problems at once:
//   constructPartialProbabilityMatrix       src/path_estimator.cpp:79-113
//   addNoiseAndNormalizeProbabilityMatrix   src/path_estimator.cpp:156-166
//   EMAbundanceEstimator                    src/path_abundance_estimator.cpp:47-114
//
// Pipeline of a solve (queueEmSolve: rpvg_hip_em_solve, and the nested model of subset_em.hip), decided by its plan
// (em_plan.hpp: planEmSolve) and queued in four stages without the host knowing the problems' sizes:
//   1. queueEmFill            the rows of every problem's cluster, cut into segments of 1 024, compacted into a per-problem
//                             CSR of row-normalised entries  P_ij/rowsum_i*(1-noise_i)  (EmProblemsView, common.hpp) at
//                             offsets the host knows (a problem keeps at most the rows and entries of its cluster):
//        fillSegmentsKernel<false>   per segment: rows and entries that survive the column subset, and the read mass of
//                                    the rows that touch no selected path
//        fillOffsetsKernel           per problem: its totals, its size bin (emBinOf) into the histogram of the work queues
//        fillSegmentsKernel<true>    per segment: the ordered compaction
//        fillDenseRowsKernel         (a few large problems, after a look at their counts) rows straight into a dense matrix
//      then emOrderKernel: the histogram becomes offsets, the problems are listed bin by bin, large first
//   2. queueEmCollapse        (with a collapse precision) readCollapseProbabilityMatrix on the problems' rows, on the
//                             collapse stream (row_collapse.hip); the EM reads the merged read counts
//   3. queueEmLaunches        the persistent launches of the plan's table, on the side streams — the bins of 64 and of 1 024
//                             threads in one launch each, whose workgroups serve one size bin for their lifetime
//                             (RPVG_HIP_EM_SEPARATE_LAUNCHES=1: one launch per kernel variant):
//        emSparseProblem<BLOCK> ONE workgroup per problem runs the whole EM loop on the GPU: abundance vector a[] and the
//                               M-step accumulators t[] live in LDS, the problem's CSR is resident in LDS or streams from
//                               L2/HBM every iteration, convergence is decided on-device
//                               (emSparseRolesKernel: bins 7, 3 and 10 in one launch; emSparseKernel: one bin)
//        emRegisterProblem      small problems dense in the registers of one wavefront
//                               (emRegisterKernel: the register bins and, merged, bin 0's sparse problems of one wavefront)
//   4. queueEmGridAndJoin     the problems of the grid bin, described to the host and solved over the whole GPU (em_grid.hip),
//                             and the join of the side streams
//
// EM iteration, fused to one pass over the rows:
//   s_i = noise_i*a_noise + sum_e P_e*a[col_e] ;  w_i = count_i / s_i
//   t[col_e] += w_i*P_e ; t_noise += w_i*noise_i
//   a'_j = a_j*t_j/T ;  a'_noise = (a_noise*t_noise + Z)/T
// where Z is the read mass of the rows without any selected path: such a row
// is (0,...,0,noise_i) after normalisation, its posterior is exactly 1 on the
// noise component for every a, so its M-step contribution is the constant
// count_i (this also subsumes what readCollapseProbabilityMatrix,
// src/path_estimator.cpp:219-259, would merge among those rows).

#include "common.hpp"

#include "collapse_plan.hpp"
#include "em_block.hpp"

#include <algorithm>
#include <memory>
#include <numeric>

using namespace rpvg_hip_detail;

namespace {

constexpr double kMinEmAbundance = 1e-8;   // src/path_abundance_estimator.cpp:11
constexpr uint32_t kMinEmConvIts = 10;     // src/path_abundance_estimator.cpp:10
static_assert(kEmBins == RPVG_HIP_EM_KERNELS, "a statistics slot per size bin (em_plan.hpp)");

// Work queues of one rpvg_hip_em_solve on the device (zero-initialised): the fill kernel counts the problems of every
// (bin, bucket); emOrderKernel turns the counts into offsets and lists the problems; the EM kernels — persistent
// workgroups — draw problems of their bin from bin_cursor until bin_count is reached.  The host never needs the counts
// to launch anything.
struct EmQueues {
    uint32_t histogram[kEmBins * kEmWorkBuckets];
    uint32_t bucket_cursor[kEmBins * kEmWorkBuckets];
    uint32_t bin_start[kEmBins];
    uint32_t bin_count[kEmBins];
    uint32_t bin_cursor[kEmBins];
    uint32_t pad;
    unsigned long long wide_cursor;   // doubles handed out of EmLaunchArgs::wide_vectors
    unsigned long long wide_overflow; // set when a wide problem did not get its vectors (capacity exceeded)
};

// ---- 1 + 2. column map, count and fill ------------------------------------------
// The rows of a problem's cluster are cut into segments of kFillSegmentRows; a work item is one segment of one problem.
// Three launches:
//   fillSegmentsKernel<false>  per item: the path -> column map of the problem in LDS (clusters of up to kLdsMapPaths
//                              paths; wider ones look their paths up in the sorted column list by bisection), then the
//                              segment's rows that touch a selected path, their entries, and the read mass — counted
//   fillOffsetsKernel          per problem: exclusive prefix of its segments' counts, the problem's totals, its size bin
//   fillSegmentsKernel<true>   per item: ordered compaction of the segment behind the rows of the segments before it
//                              (block-wide exclusive scan per 256 rows), P / rowsum * (1 - noise) with the reference's two
//                              roundings (addNoiseAndNormalizeProbabilityMatrix, src/path_estimator.cpp:156-166)
// (Round 2 and the first version of round 3: ONE workgroup per problem walked all rows of its cluster, 256 at a time, two
// block scans each — a 100 000-row cluster was 400 dependent steps and the kernel, 0.5-0.8 ms per lane, was as long as
// its largest cluster.)

struct FillArgs {
    uint32_t num_problems;                 // upper bound when num_problems_dev is set
    const uint32_t * num_problems_dev;     // null: num_problems is exact
    uint32_t num_items;                    // segments of all problems; upper bound when num_items_dev is set
    const uint32_t * num_items_dev;
    const uint64_t * seg_first;            // [P+1] first item of each problem
    const uint32_t * item_problem;         // [items]
    const uint32_t * prob_cluster;         // [P]
    const uint32_t * col_path;
    const uint64_t * cluster_row_off;
    const uint64_t * cluster_path_off;
    const uint64_t * row_ent_off;
    const uint32_t * ent_path;
    const double * ent_prob;
    const double * row_count;
    const double * row_noise;
    EmProblemsView problems;               // what the fill writes (prow_off null: count only)
    // per item: what the segment keeps (counted), then where it starts inside its problem (fillOffsetsKernel)
    uint32_t * seg_rows;
    uint32_t * seg_entries;
    double * seg_zero_mass;
    double * seg_total_mass;
    uint32_t * kept_entries;               // [P]
    uint32_t * prob_bucket;                // [P] bin * kEmWorkBuckets + bucket (with the storage only)
    EmQueues * queues;
    EmBinRule rule;
    uint32_t lds_map_paths;                // capacity of the LDS map of this launch (0: bisection for every problem)
    uint32_t long_row_scratch;             // the launch carries kFillLongRowLds bytes of LDS behind the map: clusters of long rows take a wavefront per row
    // problems whose rows are written as a dense row-major matrix instead of a CSR (the fused build: queueEmFill)
    uint32_t num_fused;
    EmFusedDense fused[kEmMaxFusedDense];
};

// whether the rows of cluster k take a wavefront each in fillSegmentsKernel
__device__ inline bool fillLongRows(const FillArgs & args, const uint32_t k) {
    const uint64_t c0 = args.cluster_row_off[k], c1 = args.cluster_row_off[k + 1];
    return emFillLongRows(args.long_row_scratch != 0, c1 - c0, args.row_ent_off[c1] - args.row_ent_off[c0]);  // (em_plan.hpp: the cluster's own size)
}

template <bool WRITE>
__global__ __launch_bounds__(256) void fillSegmentsKernel(const FillArgs args) {
    constexpr int BLOCK = 256;
    extern __shared__ __attribute__((aligned(16))) int32_t lds_map[];
    __shared__ uint32_t scratch[2 * (BLOCK / 64)];
    __shared__ double dscratch[BLOCK / 64];
    const uint32_t num_items = args.num_items_dev ? *args.num_items_dev : args.num_items;
    uint32_t mapped_problem = UINT32_MAX;
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
        const uint32_t p = args.item_problem[item];
        if (WRITE) {  // (the rows of these problems go straight into their dense matrices: fillDenseRowsKernel)
            bool fused = false;
            for (uint32_t f = 0; f < args.num_fused; ++f) fused = fused || args.fused[f].problem == p;
            if (fused) continue;
        }
        const uint32_t segment = static_cast<uint32_t>(item - args.seg_first[p]);
        const uint32_t k = args.prob_cluster[p];
        const uint32_t n_paths = static_cast<uint32_t>(args.cluster_path_off[k + 1] - args.cluster_path_off[k]);
        const uint32_t * cols = args.col_path + args.problems.col_off[p];
        const uint32_t n_cols = args.problems.paths(p);
        const bool use_map = n_paths <= args.lds_map_paths;
        // every path of the cluster is a column (the `transcripts` model: one problem per cluster over all of its paths — the column
        // list is ascending and without repeats, so as long as the cluster it is 0, 1, 2, ...): no map, and every entry is kept
        const bool identity = n_cols == n_paths;
        __syncthreads();  // (the previous item is done with the map and the scratch)
        if (use_map && !identity && mapped_problem != p) {
            for (uint32_t i = threadIdx.x; i < n_paths; i += BLOCK) lds_map[i] = -1;
            __syncthreads();
            for (uint32_t c = threadIdx.x; c < n_cols; c += BLOCK) lds_map[cols[c]] = static_cast<int32_t>(c);
            __syncthreads();
            mapped_problem = p;
        }
        auto column_of = [&](const uint32_t path) -> int32_t {
            if (identity) return static_cast<int32_t>(path);
            if (use_map) return lds_map[path];
            uint32_t lo = 0, hi = n_cols;  // first column whose path is not below `path`
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cols[mid] < path) lo = mid + 1;
                else hi = mid;
            }
            return (lo < n_cols && cols[lo] == path) ? static_cast<int32_t>(lo) : -1;
        };
        const uint64_t c0 = args.cluster_row_off[k], c1 = args.cluster_row_off[k + 1];
        const uint64_t r0 = c0 + static_cast<uint64_t>(segment) * kFillSegmentRows, r1 = min(c1, r0 + kFillSegmentRows);
        EmProblemsView::Slots at = {};
        if (WRITE) at = args.problems.slots(p);
        uint32_t * off = args.problems.prow_off + at.off;
        uint32_t run_rows = WRITE ? args.seg_rows[item] : 0, run_ent = WRITE ? args.seg_entries[item] : 0;  // (starts, by now)
        double z = 0, t = 0;  // read counts of the rows without a selected path / of all rows
        if (fillLongRows(args, k)) {
            // A cluster of long rows (the 2 000-path rows of BASELINE.json configs[1]): a wavefront per row, its lanes striding the
            // row's entries — 512-byte requests — instead of a thread walking 2 000 entries 24 KB from its neighbour's (0.2 s for
            // the 1 M x 2 000 cluster, as long as eighty EM iterations over it).  Kept entries of a row and, for the write, its
            // row sum go to LDS; the rows' places come from a scan over the segment; a row's entries are compacted 64 at a time
            // (ballot + prefix count), in order.
            uint32_t * row_n = reinterpret_cast<uint32_t *>(lds_map + args.lds_map_paths);  // [kFillSegmentRows] kept entries
            uint32_t * row_slot = row_n + kFillSegmentRows, * row_eoff = row_slot + kFillSegmentRows;  // exclusive prefixes of (kept ? 1 : 0), kept entries
            double * row_sum = reinterpret_cast<double *>(row_eoff + kFillSegmentRows);
            const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            const uint32_t seg_n = static_cast<uint32_t>(r1 - r0);
            for (uint32_t i = wave; i < seg_n; i += BLOCK / 64) {
                const uint64_t r = r0 + i;
                const uint64_t e0 = args.row_ent_off[r], e1 = args.row_ent_off[r + 1];
                uint32_t n = 0;
                double sum = 0;
                if (identity) {
                    n = static_cast<uint32_t>(e1 - e0);
                    if (WRITE) {
                        for (uint64_t e = e0 + lane; e < e1; e += 64) sum += args.ent_prob[e];
                    }
                } else {
                    for (uint64_t e = e0 + lane; e < e1; e += 64) {
                        if (column_of(args.ent_path[e]) >= 0) {
                            ++n;
                            sum += args.ent_prob[e];
                        }
                    }
                    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
                }
                if (WRITE) sum = waveSumF64(sum);
                if (lane == 0) {
                    row_n[i] = n;
                    if (WRITE) row_sum[i] = sum;
                    if (!WRITE) {
                        const double c = args.row_count[r];
                        t += c;
                        if (!n) z += c;
                    }
                }
            }
            __syncthreads();
            // exclusive scan over the segment's rows: a thread takes kFillSegmentRows / BLOCK neighbouring rows
            constexpr uint32_t kPer = kFillSegmentRows / BLOCK;
            uint32_t slots = 0, ents = 0;
            for (uint32_t j = 0; j < kPer; ++j) {
                const uint32_t i = threadIdx.x * kPer + j;
                const uint32_t n = i < seg_n ? row_n[i] : 0u;
                slots += n ? 1u : 0u;
                ents += n;
            }
            uint32_t slot0 = slots, ent0 = ents, tot_rows, tot_ent;
            blockExclusiveScanPair<BLOCK>(slot0, ent0, tot_rows, tot_ent, scratch);
            if (WRITE) {
                for (uint32_t j = 0; j < kPer; ++j) {
                    const uint32_t i = threadIdx.x * kPer + j;
                    if (i >= seg_n) break;
                    row_slot[i] = slot0;
                    row_eoff[i] = ent0;
                    slot0 += row_n[i] ? 1u : 0u;
                    ent0 += row_n[i];
                }
                __syncthreads();
                for (uint32_t i = wave; i < seg_n; i += BLOCK / 64) {
                    if (!row_n[i]) continue;
                    const uint64_t r = r0 + i;
                    const uint32_t my_row = run_rows + row_slot[i];
                    const uint32_t my_ent = run_ent + row_eoff[i];
                    const double nz = args.row_noise[r];
                    if (lane == 0) {
                        off[my_row] = my_ent;
                        args.problems.prow_count[at.row + my_row] = args.row_count[r];
                        args.problems.prow_noise[at.row + my_row] = nz;
                    }
                    const double keep = 1 - nz, rowsum = row_sum[i];
                    const uint64_t e0 = args.row_ent_off[r], e1 = args.row_ent_off[r + 1];
                    uint32_t base = 0;
                    for (uint64_t eb0 = e0; eb0 < e1; eb0 += 64) {
                        const uint64_t e = eb0 + lane;
                        const int32_t c = e < e1 ? column_of(args.ent_path[e]) : -1;
                        const unsigned long long kept = __ballot(c >= 0);
                        if (c >= 0) {
                            const uint32_t to = my_ent + base + static_cast<uint32_t>(__popcll(kept & ((1ull << lane) - 1)));
                            args.problems.pent_col[at.ent + to] = static_cast<uint32_t>(c);
                            // addNoiseAndNormalizeProbabilityMatrix: (P / rowsum) * (1 - noise), two roundings
                            args.problems.pent_val[at.ent + to] = (args.ent_prob[e] / rowsum) * keep;
                        }
                        base += static_cast<uint32_t>(__popcll(kept));
                    }
                }
            } else {
                z = blockReduceSum<double, BLOCK>(z, dscratch);
                t = blockReduceSum<double, BLOCK>(t, dscratch);
                if (threadIdx.x == 0) {
                    args.seg_rows[item] = tot_rows;
                    args.seg_entries[item] = tot_ent;
                    args.seg_zero_mass[item] = z;
                    args.seg_total_mass[item] = t;
                }
            }
            continue;
        }
        for (uint64_t rc = r0; rc < r1; rc += BLOCK) {
            const uint64_t r = rc + threadIdx.x;
            uint32_t n = 0;
            double rowsum = 0;
            uint64_t e0 = 0, e1 = 0;
            if (r < r1) {
                e0 = args.row_ent_off[r];
                e1 = args.row_ent_off[r + 1];
                for (uint64_t e = e0; e < e1; ++e) {
                    if (column_of(args.ent_path[e]) >= 0) {
                        ++n;
                        rowsum += args.ent_prob[e];
                    }
                }
                if (!WRITE) {
                    const double c = args.row_count[r];
                    t += c;
                    if (!n) z += c;
                }
            }
            uint32_t slot = n ? 1u : 0u, epos = n, tot_rows, tot_ent;
            blockExclusiveScanPair<BLOCK>(slot, epos, tot_rows, tot_ent, scratch);
            if (WRITE && n) {
                const uint32_t my_row = run_rows + slot;
                uint32_t my_ent = run_ent + epos;
                off[my_row] = my_ent;
                const double nz = args.row_noise[r];
                args.problems.prow_count[at.row + my_row] = args.row_count[r];
                args.problems.prow_noise[at.row + my_row] = nz;
                const double keep = 1 - nz;
                for (uint64_t e = e0; e < e1; ++e) {
                    const int32_t c = column_of(args.ent_path[e]);
                    if (c >= 0) {
                        args.problems.pent_col[at.ent + my_ent] = static_cast<uint32_t>(c);
                        // addNoiseAndNormalizeProbabilityMatrix: (P / rowsum) * (1 - noise), two roundings
                        args.problems.pent_val[at.ent + my_ent] = (args.ent_prob[e] / rowsum) * keep;
                        ++my_ent;
                    }
                }
            }
            run_rows += tot_rows;
            run_ent += tot_ent;
        }
        if (!WRITE) {
            z = blockReduceSum<double, BLOCK>(z, dscratch);
            t = blockReduceSum<double, BLOCK>(t, dscratch);
            if (threadIdx.x == 0) {
                args.seg_rows[item] = run_rows;
                args.seg_entries[item] = run_ent;
                args.seg_zero_mass[item] = z;
                args.seg_total_mass[item] = t;
            }
        }
    }
}

template <bool WRITE>
hipError_t launchFillSegments(const FillArgs & fa, const EmFillPlan & plan, hipStream_t st) {
    if (plan.fill_lds > kLdsOptIn) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fillSegmentsKernel<WRITE>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(plan.fill_lds));
        if (e != hipSuccess) return e;
    }
    fillSegmentsKernel<WRITE><<<dim3(plan.fill_grid), dim3(256), plan.fill_lds, st>>>(fa);
    return hipSuccess;
}

// The fused build: the rows of problem args.fused[blockIdx.y] from its cluster straight into its dense row-major matrix — what
// fillSegmentsKernel<true> and emGridDenseBuildKernel (em_grid.hip) do in two steps with the compacted CSR and a zeroed matrix
// between them, with the same arithmetic in the same order (row sum: a lane's entries in ascending order, then waveSumF64;
// value = (P / rowsum) * (1 - noise)), so the matrix is the same to the bit.  A workgroup takes segments of the cluster's rows,
// a wavefront a row at a time: the row's entries are loaded (at most 64 x kDenseRowCache: into registers, read once; longer
// rows: read twice), an image of the matrix row in LDS is zeroed meanwhile, the kept entries go to their columns of the image
// and the noise term behind the last path, and the image leaves in 16-byte stores, one behind the other.  12 B read per entry,
// 8 B written per cell, nothing written twice (zeros and values to the matrix itself: 4.1 TB/s of algorithmic bytes; the zeros
// reached HBM).
constexpr int kDenseRowCache = 32;

__global__ __launch_bounds__(256) void fillDenseRowsKernel(const FillArgs args) {
    constexpr int BLOCK = 256;
    extern __shared__ __attribute__((aligned(16))) int32_t lds_map[];
    __shared__ uint32_t scratch[2 * (BLOCK / 64)];
    const EmFusedDense fd = args.fused[blockIdx.y];
    const uint32_t p = fd.problem;
    const uint32_t k = args.prob_cluster[p];
    const uint32_t n_paths = static_cast<uint32_t>(args.cluster_path_off[k + 1] - args.cluster_path_off[k]);
    const uint32_t * cols = args.col_path + args.problems.col_off[p];
    const uint32_t n_cols = args.problems.paths(p);
    const bool identity = n_cols == n_paths;  // (fillSegmentsKernel)
    const bool use_map = !identity && n_paths <= args.lds_map_paths;
    uint32_t * row_n = reinterpret_cast<uint32_t *>(lds_map + args.lds_map_paths);  // [kFillSegmentRows] kept entries of a row
    uint32_t * row_slot = row_n + kFillSegmentRows;                                 // its place among the segment's kept rows
    double * image = reinterpret_cast<double *>(row_slot + kFillSegmentRows) + (threadIdx.x >> 6) * fd.ld;  // [ld] of this wavefront
    if (use_map) {
        for (uint32_t i = threadIdx.x; i < n_paths; i += BLOCK) lds_map[i] = -1;
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < n_cols; c += BLOCK) lds_map[cols[c]] = static_cast<int32_t>(c);
    }
    auto column_of = [&](const uint32_t path) -> int32_t {
        if (identity) return static_cast<int32_t>(path);
        if (use_map) return lds_map[path];
        uint32_t lo = 0, hi = n_cols;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cols[mid] < path) lo = mid + 1;
            else hi = mid;
        }
        return (lo < n_cols && cols[lo] == path) ? static_cast<int32_t>(lo) : -1;
    };
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t c0 = args.cluster_row_off[k], c1 = args.cluster_row_off[k + 1];
    const uint64_t rb = args.problems.slots(p).row;
    for (uint64_t item = args.seg_first[p] + blockIdx.x; item < args.seg_first[p + 1]; item += gridDim.x) {
        const uint32_t segment = static_cast<uint32_t>(item - args.seg_first[p]);
        const uint64_t r0 = c0 + static_cast<uint64_t>(segment) * kFillSegmentRows, r1 = min(c1, r0 + kFillSegmentRows);
        const uint32_t seg_n = static_cast<uint32_t>(r1 - r0);
        const uint32_t run_rows = args.seg_rows[item];  // (the segment's first row among the problem's kept rows: fillOffsetsKernel)
        __syncthreads();  // (the map is complete; the previous segment is done with the scratch)
        for (uint32_t i = wave; i < seg_n; i += BLOCK / 64) {
            const uint64_t e0 = args.row_ent_off[r0 + i], e1 = args.row_ent_off[r0 + i + 1];
            uint32_t n = static_cast<uint32_t>(e1 - e0);
            if (!identity) {
                n = 0;
                for (uint64_t e = e0 + lane; e < e1; e += 64) n += column_of(args.ent_path[e]) >= 0 ? 1u : 0u;
                for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
            }
            if (lane == 0) row_n[i] = n;
        }
        __syncthreads();
        constexpr uint32_t kPer = kFillSegmentRows / BLOCK;
        uint32_t slots = 0, unused = 0, tot_rows, tot_unused;
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t i = threadIdx.x * kPer + j;
            slots += (i < seg_n && row_n[i]) ? 1u : 0u;
        }
        uint32_t slot0 = slots;
        blockExclusiveScanPair<BLOCK>(slot0, unused, tot_rows, tot_unused, scratch);
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t i = threadIdx.x * kPer + j;
            if (i >= seg_n) break;
            row_slot[i] = slot0;
            slot0 += row_n[i] ? 1u : 0u;
        }
        __syncthreads();
        for (uint32_t i = wave; i < seg_n; i += BLOCK / 64) {
            if (!row_n[i]) continue;
            const uint64_t r = r0 + i;
            const uint32_t my_row = run_rows + row_slot[i];
            const double nz = args.row_noise[r];
            if (lane == 0) {
                args.problems.prow_count[rb + my_row] = args.row_count[r];
                args.problems.prow_noise[rb + my_row] = nz;
            }
            const double keep = 1 - nz;
            const uint64_t e0 = args.row_ent_off[r], e1 = args.row_ent_off[r + 1];
            double * out = fd.matrix + static_cast<uint64_t>(my_row) * fd.ld;
            // (a wavefront's LDS instructions execute in order: zeros, values, the read — the compiler keeps the order of accesses
            // that may touch the same words)
            for (uint32_t j = 2 * lane; j < fd.ld; j += 128) *reinterpret_cast<double2 *>(image + j) = double2{0.0, 0.0};
            if (e1 - e0 <= 64ull * kDenseRowCache) {
                int32_t col[kDenseRowCache];
                double val[kDenseRowCache];
                const uint32_t len = static_cast<uint32_t>(e1 - e0);
#pragma unroll
                for (int j = 0; j < kDenseRowCache; ++j) {
                    const uint32_t at = lane + 64u * j;
                    col[j] = -1;
                    val[j] = 0.0;
                    if (64u * j < len && at < len) {
                        col[j] = static_cast<int32_t>(args.ent_path[e0 + at]);
                        val[j] = args.ent_prob[e0 + at];
                    }
                }
                double sum = 0;
#pragma unroll
                for (int j = 0; j < kDenseRowCache; ++j) {
                    if (64u * j < len) {
                        if (col[j] >= 0) col[j] = column_of(static_cast<uint32_t>(col[j]));
                        if (col[j] >= 0) sum += val[j];
                    }
                }
                const double rowsum = waveSumF64(sum);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int j = 0; j < kDenseRowCache; ++j) {
                    // addNoiseAndNormalizeProbabilityMatrix: (P / rowsum) * (1 - noise), two roundings
                    if (64u * j < len && col[j] >= 0) image[col[j]] = (val[j] / rowsum) * keep;
                }
            } else {
                double sum = 0;
                for (uint64_t e = e0 + lane; e < e1; e += 64) {
                    if (column_of(args.ent_path[e]) >= 0) sum += args.ent_prob[e];
                }
                const double rowsum = waveSumF64(sum);
                __builtin_amdgcn_wave_barrier();
                for (uint64_t e = e0 + lane; e < e1; e += 64) {
                    const int32_t c = column_of(args.ent_path[e]);
                    if (c >= 0) image[c] = (args.ent_prob[e] / rowsum) * keep;
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) image[n_cols] = nz;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j = 2 * lane; j < fd.ld; j += 128) *reinterpret_cast<double2 *>(out + j) = *reinterpret_cast<const double2 *>(image + j);
            __builtin_amdgcn_wave_barrier();  // (the next row's zeros stay behind these reads)
        }
    }
}

// per problem: the counts of its segments become their starts; totals, terminal offset, size bin
__global__ __launch_bounds__(256) void fillOffsetsKernel(const FillArgs args) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (args.num_problems_dev ? *args.num_problems_dev : args.num_problems)) return;
    uint32_t rows = 0, entries = 0;
    double z = 0, t = 0;  // (read counts: integers, exact in any order)
    for (uint64_t item = args.seg_first[p]; item < args.seg_first[p + 1]; ++item) {
        const uint32_t r = args.seg_rows[item], e = args.seg_entries[item];
        args.seg_rows[item] = rows;
        args.seg_entries[item] = entries;
        rows += r;
        entries += e;
        z += args.seg_zero_mass[item];
        t += args.seg_total_mass[item];
    }
    if (args.problems.prow_off) {
        args.problems.prow_off[args.problems.slots(p).off + rows] = entries;
        const uint32_t n_cols = args.problems.paths(p);
        const uint32_t bucket = static_cast<uint32_t>(emBinOf(args.rule, n_cols + 1, rows, entries)) * kEmWorkBuckets + emWorkBucket(rows, entries);
        args.prob_bucket[p] = bucket;
        atomicAdd(&args.queues->histogram[bucket], 1u);
    }
    args.problems.kept_rows[p] = rows;
    args.kept_entries[p] = entries;
    args.problems.zero_mass[p] = z;
    args.problems.total_mass[p] = t;
}

// The problems of the grid bin that take the dense route (em_grid.hip) and sit on a cluster of long rows: the host gives each a
// matrix and the compaction writes their rows into it — at most kEmMaxFusedDense of them, whichever come first (the others take
// the CSR and the copy: the same matrix either way).
struct DenseCandidate {
    uint32_t problem, rows, columns, entries;
};
struct DenseCandidates {
    uint32_t count, pad;
    DenseCandidate list[kEmMaxFusedDense];
};
__global__ __launch_bounds__(256) void denseCandidatesKernel(const FillArgs args, DenseCandidates * __restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (args.num_problems_dev ? *args.num_problems_dev : args.num_problems)) return;
    if (args.prob_bucket[p] / kEmWorkBuckets != static_cast<uint32_t>(kEmGridBin)) return;
    const uint32_t columns = args.problems.paths(p) + 1;
    const uint32_t rows = args.problems.kept_rows[p], entries = args.kept_entries[p];
    if (!emDenseRule(columns, rows, entries) || !fillLongRows(args, args.prob_cluster[p])) return;
    const uint32_t at = atomicAdd(&out->count, 1u);
    if (at < static_cast<uint32_t>(kEmMaxFusedDense)) out->list[at] = DenseCandidate{p, rows, columns, entries};
}

// ---- 3. the work queues ------------------------------------------------------------
// Every workgroup scans the (bin, bucket) histogram in LDS (352 counters) and lists its problems: a problem's place
// inside its bucket is whatever the atomic hands out — the order inside a bucket only decides who starts first.
__global__ __launch_bounds__(256) void emOrderKernel(const uint32_t num_problems, const uint32_t * __restrict__ num_problems_dev,
                                                    const uint32_t * __restrict__ prob_bucket, const uint64_t * __restrict__ col_off,
                                                    EmQueues * __restrict__ queues, uint32_t * __restrict__ order,
                                                    unsigned long long * __restrict__ wide_off, const unsigned long long wide_capacity,
                                                    const uint32_t mid_grid_allowed) {
    constexpr int kCells = kEmBins * kEmWorkBuckets;
    static_assert(kCells <= 512, "two cells per thread");
    __shared__ uint32_t start[kCells + 1];
    __shared__ uint32_t wave_total[4];
    __shared__ uint32_t moved_cells;
    const uint32_t P = num_problems_dev ? *num_problems_dev : num_problems;
    // the few mid-size problems that take the grid route (above): the cells (streamed bin, buckets of 2^16 work units and more)
    // count as cells of the grid bin — every workgroup reaches the same verdict from the same histogram
    if (threadIdx.x == 0) {
        uint32_t mid = 0;
        for (uint32_t b = 0; b < kEmMidBuckets; ++b) mid += queues->histogram[kEmStreamedBin * kEmWorkBuckets + b];
        moved_cells = emMidGridMoves(mid_grid_allowed != 0, mid) ? kEmMidBuckets : 0u;
    }
    __syncthreads();
    const uint32_t moved = moved_cells;
    auto cellCount = [&](const uint32_t c) -> uint32_t {
        if (c >= kCells) return 0u;
        const uint32_t bin = c / kEmWorkBuckets, bucket = c % kEmWorkBuckets;
        if (bucket < moved && bin == kEmStreamedBin) return 0u;
        if (bucket < moved && bin == kEmGridBin) return queues->histogram[c] + queues->histogram[kEmStreamedBin * kEmWorkBuckets + bucket];
        return queues->histogram[c];
    };
    {
        // exclusive prefix of the histogram: thread t owns cells 2 t and 2 t + 1
        const uint32_t c0 = 2 * threadIdx.x, c1 = c0 + 1;
        const uint32_t h0 = cellCount(c0), h1 = cellCount(c1);
        uint32_t incl = h0 + h1;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        const uint32_t excl = before + incl - (h0 + h1);
        if (c0 < kCells) start[c0] = excl;
        if (c1 < kCells) start[c1] = excl + h0;
        if (threadIdx.x == 255) start[kCells] = before + incl;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < kEmBins) {
        queues->bin_start[threadIdx.x] = start[threadIdx.x * kEmWorkBuckets];
        queues->bin_count[threadIdx.x] = start[(threadIdx.x + 1) * kEmWorkBuckets] - start[threadIdx.x * kEmWorkBuckets];
    }
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    uint32_t cell = prob_bucket[p];
    if (cell / kEmWorkBuckets == kEmStreamedBin && cell % kEmWorkBuckets < moved) cell = kEmGridBin * kEmWorkBuckets + cell % kEmWorkBuckets;
    order[start[cell] + atomicAdd(&queues->bucket_cursor[cell], 1u)] = p;
    if (cell / kEmWorkBuckets == 10) {  // abundance + accumulator vectors in global memory
        const unsigned long long need = 2ull * (static_cast<unsigned long long>(col_off[p + 1] - col_off[p]) + 1);
        const unsigned long long at = atomicAdd(&queues->wide_cursor, need);
        wide_off[p] = at;
        if (at + need > wide_capacity) atomicAdd(&queues->wide_overflow, 1ull);
    }
}

// ---- 4. the problems of the grid bin, described to the host ----------------------------------------
// The grid bin has no kernel of its own here: its problems are solved over the whole GPU with one round of launches per
// EM iteration, which the host drives (em_grid.hip).  One thread per problem of the bin writes what the host needs.
struct GridDescribeArgs {
    const EmQueues * queues;
    const uint32_t * order;
    EmProblemsView problems;
    const uint32_t * kept_entries;
    EmGridProblem * out;
    uint32_t capacity;
};

__global__ __launch_bounds__(256) void emGridDescribeKernel(const GridDescribeArgs args) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= args.queues->bin_count[kEmGridBin] || i >= args.capacity) return;
    const uint32_t p = args.order[args.queues->bin_start[kEmGridBin] + i];
    EmGridProblem d;
    d.problem = p;
    const EmProblemsView & v = args.problems;
    d.columns = v.paths(p) + 1;
    d.rows = v.kept_rows[p];
    d.entries = args.kept_entries[p];
    d.merged = (v.problem_merged != nullptr && v.problem_merged[p] != 0) ? 1u : 0u;
    d.pad = 0;
    d.row_base = v.row_base[p];
    d.ent_base = v.ent_base[p];
    d.col_begin = v.col_off[p];
    d.total_mass = v.total_mass[p];
    d.zero_mass = v.zero_mass[p];
    args.out[i] = d;
}

// ---- 5. the EM kernel --------------------------------------------------------

struct EmLaunchArgs {
    const uint32_t * order;        // problems, bin by bin (EmQueues::bin_start), large first
    EmQueues * queues;
    uint32_t bin;                  // the bin this launch serves
    EmProblemsView problems;       // (with the merged read counts of a collapse)
    uint32_t max_em_its;
    uint32_t register_copies;      // emRegisterKernel<1,16>: small problems in copies (RPVG_HIP_EM_COPIES=0: never)
    double max_rel_em_conv;
    double * wide_vectors;         // problems too wide for LDS: abundance + accumulator vectors, 2 C doubles each,
    const unsigned long long * wide_off;  // [P] at this offset (emSparseKernel<..., WIDE>)
    unsigned long long wide_capacity;
    double * abundances;           // [col_off[P]]
    double * noise_count;          // [P]
    uint32_t * iterations;         // [P]
};

// The EM kernels are persistent: a launch has as many workgroups as the GPU holds at once (or as the bin can have
// problems, if fewer), and every workgroup draws the next problem of its bin from the queue until the bin is empty —
// the host launches every variant without knowing how many problems each bin got.  Returns the problem, or
// UINT32_MAX when the bin is exhausted; uniform over the workgroup.
template <int BLOCK>
__device__ __forceinline__ uint32_t nextProblem(const EmLaunchArgs & args, uint32_t * slot) {
    uint32_t i;
    if (BLOCK == 64) {
        i = (threadIdx.x == 0) ? atomicAdd(&args.queues->bin_cursor[args.bin], 1u) : 0u;
        i = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(i)));
    } else {
        __syncthreads();  // everybody is done with the previous problem (and with *slot)
        if (threadIdx.x == 0) *slot = atomicAdd(&args.queues->bin_cursor[args.bin], 1u);
        __syncthreads();
        i = *slot;
    }
    if (i >= args.queues->bin_count[args.bin]) return UINT32_MAX;
    return args.order[args.queues->bin_start[args.bin] + i];
}

// RESIDENT: the problem's compacted CSR is copied into LDS once and every EM iteration runs out of LDS
// (small problems need up to thousands of iterations; from L2 each costs ~1.7 us of dependent-load
// latency, from LDS a fraction of that).
// WIDE: the abundance and accumulator vectors do not fit LDS (C >= 3 993 columns: the reference's EM has no
// size limit, and clusters such as HLA exceed this): they live in global memory (L2), the M-step uses global FP64 atomics.
template <int BLOCK, bool RESIDENT, bool WIDE>
__device__ __forceinline__ void emSparseProblem(const EmLaunchArgs & args, const uint32_t p, unsigned char * smem_raw) {
    const uint32_t C = args.problems.paths(p) + 1;  // + noise
    if (WIDE && args.wide_off[p] + 2ull * C > args.wide_capacity) return;  // (reported through EmQueues::wide_overflow)
    // The M-step's column sums have ONE order of additions, whatever the wavefronts' timing: every wavefront adds into an
    // accumulator vector of its own — within a wavefront the additions follow the program and, lanes of one instruction that meet on
    // a column, the LDS unit's lane order — and the vectors are added up in wavefront order (registers -> LDS slots -> ordered
    // sum).  Two runs on the same input give the same bits, iteration counts included.  (WIDE — more than ~3 900 columns, the
    // vectors in global memory — keeps one vector and global atomics: reproducible up to the order of those additions.)
    constexpr uint32_t kCopies = WIDE ? 1 : BLOCK / 64;
    double * a = WIDE ? args.wide_vectors + args.wide_off[p] : reinterpret_cast<double *>(smem_raw);  // [C] abundances (last = noise)
    double * t = a + C;                                 // [kCopies x C] M-step accumulators
    double * red = WIDE ? reinterpret_cast<double *>(smem_raw) : t + static_cast<size_t>(kCopies) * C;  // [BLOCK/64] reduction scratch
    double * tw = t + static_cast<size_t>(kCopies == 1 ? 0 : threadIdx.x >> 6) * C;  // this wavefront's

    const EmProblemRows csr = args.problems.mergedRows(p);
    const uint32_t n_rows = csr.rows;
    const uint32_t * off = csr.off;
    const double * cnt = csr.count;
    const double * nzv = csr.noise;
    const uint32_t * col = csr.col;
    const double * val = csr.val;
    if (RESIDENT) {
        const uint32_t n_ent = off[n_rows];
        double * l_cnt = red + (BLOCK / 64 + 2);
        double * l_nz = l_cnt + n_rows;
        double * l_val = l_nz + n_rows;
        uint32_t * l_off = reinterpret_cast<uint32_t *>(l_val + n_ent);
        uint32_t * l_col = l_off + (n_rows + 1);
        for (uint32_t r = threadIdx.x; r < n_rows; r += BLOCK) {
            l_cnt[r] = cnt[r];
            l_nz[r] = nzv[r];
        }
        for (uint32_t r = threadIdx.x; r <= n_rows; r += BLOCK) l_off[r] = off[r];
        for (uint32_t e = threadIdx.x; e < n_ent; e += BLOCK) {
            l_val[e] = val[e];
            l_col[e] = col[e];
        }
        off = l_off;
        cnt = l_cnt;
        nzv = l_nz;
        col = l_col;
        val = l_val;
    }
    const double T = args.problems.total_mass[p];
    const double Z = args.problems.zero_mass[p];
    const double eps = args.max_rel_em_conv;
    const uint32_t noise_col = C - 1;

    // src/path_abundance_estimator.cpp:54 — 1 / float(C), widened
    const double a0 = static_cast<double>(1.0f / static_cast<float>(C));
    for (uint32_t j = threadIdx.x; j < C; j += BLOCK) a[j] = a0;

    for (uint32_t j = threadIdx.x; j < kCopies * C; j += BLOCK) t[j] = 0;
    __syncthreads();  // a[], t[] and (when resident) the problem's CSR are in LDS

    const double inv_T = 1.0 / T;
    uint32_t iters = 0, conv = 0;
    for (uint32_t it = 0; it < args.max_em_its; ++it) {
        const double a_noise = a[noise_col];
        double tn = 0;
        for (uint32_t r = threadIdx.x; r < n_rows; r += BLOCK) {
            const uint32_t e0 = off[r], e1 = off[r + 1];
            const double nz = nzv[r];
            double s = nz * a_noise;
            for (uint32_t e = e0; e < e1; ++e) s += val[e] * a[col[e]];
            // cnt / s: hardware reciprocal, two Newton steps, one residual correction of the quotient
            double y = __builtin_amdgcn_rcp(s);
            y = fma(fma(-s, y, 1.0), y, y);
            y = fma(fma(-s, y, 1.0), y, y);
            const double quot = cnt[r] * y;
            // (a row whose count a row collapse moved to its run head takes no part: row_collapse.hip)
            const double w = cnt[r] == 0.0 ? 0.0 : fma(fma(-s, quot, cnt[r]), y, quot);
            for (uint32_t e = e0; e < e1; ++e) atomicAdd(&tw[col[e]], w * val[e]);
            tn += w * nz;
        }
        // the noise column has no entries: its accumulator takes the per-wave sums of w * noise
        tn = waveSumF64(tn);
        if ((threadIdx.x & 63) == 0 && tn != 0.0) atomicAdd(&tw[noise_col], tn);
        __syncthreads();  // all atomics to t[] done, all reads of a[] done
        int viol = 0;
        for (uint32_t j = threadIdx.x; j < C; j += BLOCK) {
            const double aj = a[j];
            double tj = t[j];
            t[j] = 0;
#pragma unroll
            for (uint32_t w = 1; w < kCopies; ++w) {  // (wavefront order)
                tj += t[w * C + j];
                t[w * C + j] = 0;
            }
            const double an = (j == noise_col) ? (aj * tj + Z) * inv_T : (aj * tj) * inv_T;
            // |an - aj| / an > eps  (src/path_abundance_estimator.cpp:73-75), without the division
            if (an >= kMinEmAbundance && fabs(an - aj) > eps * an) viol = 1;
            a[j] = an;
        }
        int any_viol;
        if (BLOCK == 64) {
            any_viol = __any(viol);
            __syncthreads();
        } else {
            any_viol = __syncthreads_or(viol);
        }
        ++iters;
        if (!any_viol) {
            if (++conv == kMinEmConvIts) break;
        } else {
            conv = 0;
        }
    }

    // src/path_abundance_estimator.cpp:100-113
    double low = 0;
    double * out = args.abundances + args.problems.col_off[p];
    for (uint32_t j = threadIdx.x; j < noise_col; j += BLOCK) {
        const double aj = a[j];
        if (aj < kMinEmAbundance) {
            low += aj * T;
            out[j] = 0;
        } else {
            out[j] = aj * T;
        }
    }
    low = blockReduceSum<double, BLOCK>(low, red);
    if (threadIdx.x == 0) {
        args.noise_count[p] = low + a[noise_col] * T;
        args.iterations[p] = iters;
    }
}

// the bin of a role (selects, not an indexed read: the table stays in the launch's arguments)
__device__ __forceinline__ uint32_t roleBin(const EmRoles & roles, const uint32_t role) {
    uint32_t bin = roles.bin[0];
#pragma unroll
    for (uint32_t v = 1; v < kEmMaxRoles; ++v) bin = v == role ? roles.bin[v] : bin;
    return bin;
}

// workgroup `block` of the ones that serve args.bin (the whole workgroup: every barrier inside is uniform over it)
template <int BLOCK, bool RESIDENT, bool WIDE = false>
__device__ __forceinline__ void emSparseBin(const EmLaunchArgs & args, const uint32_t block, unsigned char * smem_raw, uint32_t * next_slot) {
    if (block >= args.queues->bin_count[args.bin]) return;  // more workgroups than the bin has problems
    for (uint32_t p = nextProblem<BLOCK>(args, next_slot); p != UINT32_MAX; p = nextProblem<BLOCK>(args, next_slot)) {
        emSparseProblem<BLOCK, RESIDENT, WIDE>(args, p, smem_raw);
        if (BLOCK == 64) __syncthreads();  // (the LDS is reused; wider workgroups meet in nextProblem)
    }
}

template <int BLOCK, bool RESIDENT, bool WIDE = false>
__global__ __launch_bounds__(BLOCK) void emSparseKernel(const EmLaunchArgs args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ uint32_t next_slot;
    emSparseBin<BLOCK, RESIDENT, WIDE>(args, blockIdx.x, smem_raw, &next_slot);
}

// The bins of 1 024 threads in ONE launch (the plan's merged launches: emLaunchRoles): a workgroup serves one bin for its lifetime —
// role blockIdx.x % variants, as that bin's workgroup blockIdx.x / variants — with that bin's code, guard and cursor: no workgroup mixes roles,
// so every barrier stays uniform over its workgroup, and a problem's arithmetic is what its own launch did.  Bins 7 and 3, and with
// WITH_WIDE bin 10 — a kernel of its own, for the solves that can have such a problem: the wide variant's code costs the others
// registers (profiles/em_launches/resource_usage.txt).
template <bool WITH_WIDE>
__global__ __launch_bounds__(1024) void emSparseRolesKernel(const EmLaunchArgs launch_args, const EmRoles roles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ uint32_t next_slot;
    const uint32_t role = blockIdx.x % roles.variants, block = blockIdx.x / roles.variants;
    EmLaunchArgs args = launch_args;
    const uint32_t bin = roleBin(roles, role);
    // (the bin a constant inside each role's code, as it is a launch argument in a launch of its own)
    if (bin == kSparse1024Bins[0]) {
        args.bin = kSparse1024Bins[0];
        emSparseBin<1024, true>(args, block, smem_raw, &next_slot);
    } else if (bin == kSparse1024Bins[1]) {
        args.bin = kSparse1024Bins[1];
        emSparseBin<1024, false>(args, block, smem_raw, &next_slot);
    } else if (WITH_WIDE && bin == kSparse1024Bins[2]) {
        args.bin = kSparse1024Bins[2];
        emSparseBin<1024, false, true>(args, block, smem_raw, &next_slot);
    }
}

// `grid`: workgroups of the persistent launch (the caller's bound on the problems of the bin, capped by what the GPU holds)
template <int BLOCK, bool RESIDENT, bool WIDE = false>
hipError_t launchEm(const EmLaunchArgs & args, uint32_t grid, size_t lds, hipStream_t stream) {
    if (grid == 0) return hipSuccess;
    if (lds > kLdsOptIn) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&emSparseKernel<BLOCK, RESIDENT, WIDE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    emSparseKernel<BLOCK, RESIDENT, WIDE><<<dim3(grid), dim3(BLOCK), lds, stream>>>(args);
    return hipGetLastError();
}

// `lds`: the largest of the roles' dynamic LDS
template <bool WITH_WIDE>
hipError_t launchEmRoles(const EmLaunchArgs & args, const EmRoles & roles, size_t lds, hipStream_t stream) {
    const uint32_t grid = roles.variants * roles.grid;
    if (grid == 0) return hipSuccess;
    if (lds > kLdsOptIn) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&emSparseRolesKernel<WITH_WIDE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    emSparseRolesKernel<WITH_WIDE><<<dim3(grid), dim3(1024), lds, stream>>>(args, roles);
    return hipGetLastError();
}


// ---- register-resident EM for small problems ---------------------------------------------------------------
// A problem with at most COLS columns — its paths AND the noise component — and 64 * RPL rows is held DENSE in the
// registers of one wavefront: lane l owns rows l, l + 64, ... (RPL of them) as COLS doubles each, the noise probability
// of the row in the column behind the last path.  An iteration then needs no dependent memory access for the matrix:
// the E-step is RPL x COLS fused multiply-adds against the abundance vector, the M-step RPL x COLS more into COLS
// per-lane partial column sums, which cross the wave once through LDS (64 / COLS lanes per column + one or two DPP
// steps inside the quad).  These problems are the ones that run for thousands of iterations (the batch's EM time is the
// iteration count of its slowest problem times the latency of ONE iteration — a 14-path, 17-row problem with 2 494 of
// them in the configs[2] bench).  Zero entries add exact zeros; the column sums are added in a fixed order (the sparse
// kernels use LDS atomics).  Round 3: the noise component became a column like the others (it was a wave-wide DPP sum
// of its own next to the transposition: 27 instructions of ~230 per iteration), the update runs in every lane of a
// column without a branch, and the transposition is skewed (below).
// value of the lane whose index differs in bit 0 (D = 1) or bit 1 (D = 2) — inside a quad, through DPP
template <int D>
__device__ __forceinline__ double quadSwapF64(const double v) {
    constexpr int perm = (D == 1) ? 0xB1 : 0x4E;  // quad_perm [1,0,3,2] / [2,3,0,1]
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), perm, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), perm, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// x of the lanes 32 .. 63 <-> y of the lanes 0 .. 31 (v_permlane32_swap_b32, new with gfx950): afterwards x + y is, in a lane
// of the lower half, the sum of the two x of the lanes l and l + 32, in a lane of the upper half that of the two y
__device__ __forceinline__ void swapHalvesF64(double & x, double & y) {
    const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(__double2loint(x)), static_cast<unsigned>(__double2loint(y)), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(__double2hiint(x)), static_cast<unsigned>(__double2hiint(y)), false, false);
    x = __hiloint2double(static_cast<int>(hi[0]), static_cast<int>(lo[0]));
    y = __hiloint2double(static_cast<int>(hi[1]), static_cast<int>(lo[1]));
}

// the same between neighbouring rows of 16 lanes: x of the odd rows <-> y of the even rows (v_permlane16_swap_b32)
__device__ __forceinline__ void swapRowsF64(double & x, double & y) {
    const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(__double2loint(x)), static_cast<unsigned>(__double2loint(y)), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(__double2hiint(x)), static_cast<unsigned>(__double2hiint(y)), false, false);
    x = __hiloint2double(static_cast<int>(hi[0]), static_cast<int>(lo[0]));
    y = __hiloint2double(static_cast<int>(hi[1]), static_cast<int>(lo[1]));
}

// One halving step inside a row of 16 lanes: the DPP control CTRL pairs every lane with one whose `upper` differs; a
// lane keeps x (upper: y) and adds the partner's copy of it.
template <int CTRL>
__device__ __forceinline__ double halveF64(const double x, const double y, const bool upper) {
    const double send = upper ? x : y, keep = upper ? y : x;
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(send), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(send), CTRL, 0xF, 0xF, true);
    return keep + __hiloint2double(hi, lo);
}

// Column sums over the wave of COLS per-lane partials v[0 .. COLS), without LDS: every step halves the number of values
// a lane carries and doubles the lanes each value has been added over — lanes l and l + 32 (one swap per 32-bit
// register half and one addition for TWO columns), neighbouring rows of 16 lanes, then inside the row through DPP.
// Afterwards lane l holds, in the return value, the sum of column l / (64 / COLS) over all 64 lanes; the order of the
// additions is fixed.  (Round 2 and the first version of round 3 transposed the partials through LDS: 16 writes and 16
// reads per lane, 625 of an iteration's 1 180 cycles in LDS issue and waits — PMC, tools/r03_em_pmc.sh.)
// SKIP: the first SKIP halving steps have nothing to add (problems of at most 32 / 16 rows whose lanes 32 .. 63 / 16 .. 63 carry
// copies of the rows, every copy the partial sums of its share of the columns in v[0 .. COLS >> SKIP): exactly where those steps
// would have put them, the other addends being zeros).
template <int COLS, int SKIP = 0>
__device__ __forceinline__ double columnSumsOverWave(double (&v)[COLS], const uint32_t lane) {
    if (SKIP < 1) {
#pragma unroll
        for (int c = 0; c < COLS / 2; ++c) {
            swapHalvesF64(v[c], v[c + COLS / 2]);
            v[c] += v[c + COLS / 2];
        }
    }
    if (SKIP < 2) {
#pragma unroll
        for (int c = 0; c < COLS / 4; ++c) {
            swapRowsF64(v[c], v[c + COLS / 4]);
            v[c] += v[c + COLS / 4];
        }
    }
    const bool bit3 = (lane & 8) != 0, bit2 = (lane & 4) != 0;
#pragma unroll
    for (int c = 0; c < COLS / 8; ++c) v[c] = halveF64<0x128>(v[c], v[c + COLS / 8], bit3);   // row_ror:8
#pragma unroll
    for (int c = 0; c < COLS / 16; ++c) v[c] = halveF64<0x141>(v[c], v[c + COLS / 16], bit2);  // row_half_mirror
    double t;
    if (COLS == 32) {
        t = halveF64<0x4E>(v[0], v[1], (lane & 2) != 0);  // quad_perm [2,3,0,1]
    } else {
        t = v[0];
        t += quadSwapF64<2>(t);
    }
    t += quadSwapF64<1>(t);
    return t;
}

// COPIES (one row per lane, 16 columns): a problem of at most 64 / COPIES rows is held COPIES times — lane l carries row
// l % (64 / COPIES) — and every copy takes 16 / COPIES of the columns in the M-step: 16 / COPIES multiplications instead of 16, and
// the first log2(COPIES) steps of the column sums (eight and four swaps and additions) fall away.  The E-step, and with it every
// value, is what it is with one copy (the steps left out add zeros).  The batch's EM time is the latency of one iteration times
// the iterations of its slowest problems, and those are small (2 268 iterations on 17 rows in the configs[2] batch).
template <int RPL, int COLS, int COPIES = 1>
__device__ __forceinline__ void emRegisterProblem(const EmLaunchArgs & args, const uint32_t p, double * reg_lds) {
    static_assert(COPIES == 1 || (RPL == 1 && COLS == 16), "copies: one row per lane, 16 columns");
    constexpr uint32_t kCols = COLS;
    constexpr int kSkip = COPIES == 4 ? 2 : (COPIES == 2 ? 1 : 0);
    constexpr int kShare = COLS / COPIES;  // columns of a copy in the M-step
    constexpr int kLanesPerColumn = 64 / COLS;  // 4 (16 columns) or 2 (32 columns)
    const uint32_t np = args.problems.paths(p);  // < kCols; column np = noise
    const uint32_t lane = threadIdx.x;
    const EmProblemRows csr = args.problems.mergedRows(p);
    const uint32_t n_rows = csr.rows;
    const uint32_t * off = csr.off;
    const double * cnt = csr.count;
    const double * nzv = csr.noise;
    const uint32_t * col = csr.col;
    const double * val = csr.val;

    // stage the dense tile through LDS (the scatter needs dynamic indexing, registers must not)
    constexpr uint32_t kTile = 64 * RPL * kCols;
    double * tile = reg_lds;
    for (uint32_t idx = lane; idx < kTile; idx += 64) tile[idx] = 0.0;
    __syncthreads();
    for (uint32_t r = lane; r < n_rows; r += 64) {
        for (uint32_t e = off[r]; e < off[r + 1]; ++e) tile[r * kCols + col[e]] += val[e];
        tile[r * kCols + np] = nzv[r];
    }
    __syncthreads();
    double P[RPL][kCols], c[RPL];
    double mine[kShare];  // (COPIES > 1) the row's values in the columns of this copy
    bool valid[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const uint32_t r = COPIES > 1 ? lane % (64 / COPIES) : q * 64 + lane;
        c[q] = r < n_rows ? cnt[r] : 0.0;
        valid[q] = c[q] != 0.0;  // (also: a row whose count a row collapse moved to its run head, row_collapse.hip)
#pragma unroll
        for (int j = 0; j < static_cast<int>(kCols); ++j) P[q][j] = tile[r * kCols + j];
        if (COPIES > 1) {
            const uint32_t first_column = (lane / (64 / COPIES)) * kShare;
#pragma unroll
            for (int j = 0; j < kShare; ++j) mine[j] = tile[r * kCols + first_column + j];
        }
    }
    const double T = args.problems.total_mass[p];
    const double eps = args.max_rel_em_conv;
    // src/path_abundance_estimator.cpp:54 — 1 / float(C), widened
    const double a0 = static_cast<double>(1.0f / static_cast<float>(np + 1));
    // Column j belongs to lanes kLanesPerColumn * j ...: each holds a_j and applies the update (the same arithmetic on the
    // same values: no lane is special, nothing branches).  Columns behind the noise column are padding: their
    // abundance starts, and therefore stays, at zero.
    const uint32_t my_col = lane / kLanesPerColumn;
    double a_mine = (my_col <= np) ? a0 : 0.0;
    // Z: the read mass of the rows without any selected path, which the noise component takes whole (header of this file)
    const double z_mine = (my_col == np) ? args.problems.zero_mass[p] : 0.0;

    const double inv_T = 1.0 / T;

    uint32_t iters = 0, conv = 0;
    for (uint32_t it = 0; it < args.max_em_its; ++it) {
        // the abundance vector lives in its owner lanes (a_mine): read straight from them (scalar broadcast)
        double av[kCols];
#pragma unroll
        for (int j = 0; j < static_cast<int>(kCols); ++j) av[j] = readLaneF64(a_mine, j * kLanesPerColumn);
        double w[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            // four interleaved partial sums: the latency of one iteration is what this kernel is about
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int j = 0; j < static_cast<int>(kCols); j += 4) {
                s0 = fma(P[q][j], av[j], s0);
                s1 = fma(P[q][j + 1], av[j + 1], s1);
                s2 = fma(P[q][j + 2], av[j + 2], s2);
                s3 = fma(P[q][j + 3], av[j + 3], s3);
            }
            const double s = (s0 + s1) + (s2 + s3);
            // c / s: hardware reciprocal, two Newton steps, one residual correction of the quotient
            double y = __builtin_amdgcn_rcp(s);
            y = fma(fma(-s, y, 1.0), y, y);
            y = fma(fma(-s, y, 1.0), y, y);
            const double quot = c[q] * y;
            w[q] = valid[q] ? fma(fma(-s, quot, c[q]), y, quot) : 0.0;
        }
        double pj[kCols];
        if (COPIES > 1) {
#pragma unroll
            for (int j = 0; j < kShare; ++j) pj[j] = w[0] * mine[j];
        } else {
#pragma unroll
            for (int j = 0; j < static_cast<int>(kCols); ++j) {
                pj[j] = w[0] * P[0][j];
#pragma unroll
                for (int q = 1; q < RPL; ++q) pj[j] = fma(w[q], P[q][j], pj[j]);
            }
        }
        const double tj = columnSumsOverWave<COLS, kSkip>(pj, lane);

        // a'_j = a_j t_j / T;  a'_noise = (a_noise t_noise + Z) / T  (z_mine is zero off the noise column)
        const double an = fma(a_mine, tj, z_mine) * inv_T;
        // |an - aj| / an > eps  (src/path_abundance_estimator.cpp:73-75), without the division
        const bool viol = (an >= kMinEmAbundance) & (fabs(an - a_mine) > eps * an);
        a_mine = an;
        const int any_viol = __any(viol);
        ++iters;
        if (!any_viol) {
            if (++conv == kMinEmConvIts) break;
        } else {
            conv = 0;
        }
    }

    // src/path_abundance_estimator.cpp:100-113
    double low = 0.0;
    const bool first_of_column = (lane % kLanesPerColumn) == 0;
    if (first_of_column && my_col < np) {
        double * out = args.abundances + args.problems.col_off[p];
        if (a_mine < kMinEmAbundance) {
            low = a_mine * T;
            out[my_col] = 0;
        } else {
            out[my_col] = a_mine * T;
        }
    }
    low = waveSumF64(low);
    if (first_of_column && my_col == np) {
        args.noise_count[p] = low + a_mine * T;
        args.iterations[p] = iters;
    }
}

// workgroup `block` of the ones that serve args.bin
template <int RPL, int COLS>
__device__ __forceinline__ void emRegisterBin(const EmLaunchArgs & args, const uint32_t block, double * reg_lds) {
    if (block >= args.queues->bin_count[args.bin]) return;  // more workgroups than the bin has problems
    // (RPVG_HIP_EM_COPIES=0 in the launch arguments: every problem with one copy, A/B and tests)
    for (uint32_t p = nextProblem<64>(args, nullptr); p != UINT32_MAX; p = nextProblem<64>(args, nullptr)) {
        if (RPL == 1 && COLS == 16 && args.register_copies) {
            const uint32_t n_rows = args.problems.kept_rows[p];
            if (n_rows <= 16) emRegisterProblem<1, 16, 4>(args, p, reg_lds);
            else if (n_rows <= 32) emRegisterProblem<1, 16, 2>(args, p, reg_lds);
            else emRegisterProblem<1, 16, 1>(args, p, reg_lds);
        } else {
            emRegisterProblem<RPL, COLS>(args, p, reg_lds);
        }
        __syncthreads();  // the staging tile is reused
    }
}

// one launch per bin (RPVG_HIP_EM_REGISTER_LAUNCHES=5: A/B, and the per-bin device times of rpvg_hip_kernel_stats)
template <int RPL, int COLS>
__global__ __launch_bounds__(64) void emRegisterBinKernel(const EmLaunchArgs args) {
    extern __shared__ __attribute__((aligned(16))) double reg_lds[];
    emRegisterBin<RPL, COLS>(args, blockIdx.x, reg_lds);
}

// The register-resident bins in ONE launch: workgroup b serves bin kRegisterBins[b % variants] as that bin's workgroup
// b / variants (the variants side by side from the first workgroup on).  A launch lasts as long as its slowest problem iterates
// — a millisecond per bin on the configs[2] batch, on a few wavefronts —, and launches that share a stream, or, with batches
// in flight, a hardware queue with other contexts' streams, run one after the other: five bins in five launches were 4.1 ms
// of queue time per batch, in one launch they are 1.3.
// The wave launch of the plan's merged launches adds bin 0 — the LDS-resident sparse problems of one wavefront, emSparseProblem<64,
// true> — as one more role: its 8 KB lie inside the staging tile.  (`roles`: emLaunchRoles.)
// (kRegisterBins, kRegisterKernelIndex: em_plan.hpp)

__global__ __launch_bounds__(64) void emRegisterKernel(const EmLaunchArgs launch_args, const EmRoles roles) {
    extern __shared__ __attribute__((aligned(16))) double reg_lds[];
    EmLaunchArgs args = launch_args;
    const uint32_t role = blockIdx.x % roles.variants, block = blockIdx.x / roles.variants;
    args.bin = roleBin(roles, role);
    switch (args.bin) {
        case 6: emRegisterBin<4, 16>(args, block, reg_lds); break;
        case 4: emRegisterBin<1, 16>(args, block, reg_lds); break;
        case 5: emRegisterBin<2, 16>(args, block, reg_lds); break;
        case 8: emRegisterBin<1, 32>(args, block, reg_lds); break;
        case 9: emRegisterBin<2, 32>(args, block, reg_lds); break;
        case kWaveSparseBin: emSparseBin<64, true>(args, block, reinterpret_cast<unsigned char *>(reg_lds), nullptr); break;
        default: break;
    }
}

template <int RPL, int COLS>
hipError_t launchEmRegister(const EmLaunchArgs & args, uint32_t grid, size_t lds, hipStream_t stream) {  // lds: the staging tile
    if (grid == 0) return hipSuccess;
    emRegisterBinKernel<RPL, COLS><<<dim3(grid), dim3(64), lds, stream>>>(args);
    return hipGetLastError();
}

// the register bins (three without problems of more than 16 columns, else five), and bin 0 in the wave launch: the roles' grids
hipError_t launchEmRegisterBins(const EmLaunchArgs & args, const EmRoles & roles, const size_t lds, hipStream_t stream) {
    const uint32_t grid = roles.variants * roles.grid;
    if (grid == 0) return hipSuccess;
    emRegisterKernel<<<dim3(grid), dim3(64), lds, stream>>>(args, roles);
    return hipGetLastError();
}

}  // namespace

namespace rpvg_hip_detail {

size_t emQueuesBytes() { return sizeof(EmQueues); }
uint32_t emFillSegmentRows() { return kFillSegmentRows; }

// The environment of a solve.  Names read per call stay per call (the tests switch them inside one process), the others are
// read once per process; the names behind RPVG_EXPERIMENT_ENV exist in an EXPERIMENTS=1 build only (docs/design/knobs.md).
EmSolveKnobs emSolveKnobs() {
    static const EmSolveKnobs once = []() {
        EmSolveKnobs k;
        k.rule.use_register_kernel = RPVG_EXPERIMENT_ENV("RPVG_HIP_NO_REGISTER_EM") == nullptr ? 1u : 0u;
        // A streamed problem is one workgroup: above this many rows + entries it gets 1 024 threads instead of 256 (round 2:
        // 262 144 — a 200 000-entry problem on 256 threads took 47 us per EM iteration and, at 23 iterations, as long as the
        // thousands of iterations of the slowest register-resident problem; round 3: 24 576, then 0 — a batch has a few dozen
        // streamed problems, far fewer than CUs, and on 256 threads the ones below the limit took 55 us per iteration, twice
        // what the larger ones above it took on 1 024).
        k.rule.streamed_small_work = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_STREAM_SMALL") ? std::strtoull(RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_STREAM_SMALL"), nullptr, 10) : 0;
        k.no_collapse = RPVG_EXPERIMENT_ENV("RPVG_HIP_NO_EM_COLLAPSE") != nullptr;
        const char * launches = std::getenv("RPVG_HIP_EM_REGISTER_LAUNCHES");
        k.one_register_launch = !(launches && std::atoi(launches) == 5);
        k.fill_thread_rows = RPVG_EXPERIMENT_ENV("RPVG_HIP_FILL_THREAD_ROWS") != nullptr;  // A/B knob
        k.grid_scale = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_GRID_SCALE") ? std::atof(RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_GRID_SCALE")) : 1.0;  // A/B knob
        k.few_streams = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_FEW_STREAMS") != nullptr;  // A/B knob
        k.launch_early = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_LAUNCH_EARLY") != nullptr;  // A/B: queue the EM launches without waiting for the collapse
        k.wait_sort_only = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_WAIT_SORT_ONLY") != nullptr;  // A/B: only the collapse's sort (11.3 against 10.2 ms per batch)
        k.join_on_stream = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_JOIN_ON_STREAM") != nullptr;  // A/B: the context's stream waits for the side streams, not the thread
        k.collapse_debug = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_COLLAPSE_DEBUG") != nullptr;
        return k;
    }();
    EmSolveKnobs k = once;
    k.rule.grid_min_work = emGridMinWork();  // RPVG_HIP_EM_GRID_MIN_WORK
    k.no_collapse = k.no_collapse || RPVG_EXPERIMENT_ENV("RPVG_HIP_NO_COLLAPSE") != nullptr;
    k.no_fused_dense = std::getenv("RPVG_HIP_NO_FUSED_DENSE") != nullptr;
    // the bins of 64 and of 1 024 threads in one launch each (planEmSolve); RPVG_HIP_EM_SEPARATE_LAUNCHES=1: a launch per kernel variant (A/B and tests)
    const char * separate = std::getenv("RPVG_HIP_EM_SEPARATE_LAUNCHES");
    k.merged_launches = !(separate && std::atoi(separate) != 0);
    const char * copies = std::getenv("RPVG_HIP_EM_COPIES");
    k.register_copies = copies ? std::atoi(copies) != 0 : true;
    // (storage by the bound up to this budget; by default two fifths of the free device memory and at most 32 GiB: prepareHostProblems)
    const char * budget = std::getenv("RPVG_HIP_EM_BOUND_BYTES");
    k.has_bound_bytes = budget != nullptr;
    k.bound_bytes = budget ? static_cast<uint64_t>(std::atof(budget)) : 0;
    return k;
}

EmSolveShape emSolveShape(const rpvg_hip_ctx * ctx, const EmProblemList & list, const bool collapse_wanted) {
    EmSolveShape s;
    s.P = list.P_bound;
    s.items_bound = list.items_bound;
    s.max_cols = list.max_cols;
    s.max_cluster_paths = list.max_cluster_paths;
    s.max_cluster_work = list.max_cluster_work;
    s.rows_capacity = list.rows_capacity;
    s.wide_capacity = list.wide_capacity;
    s.cus = static_cast<uint32_t>(ctx->props.multiProcessorCount);
    s.side_streams = ctx->aux_count;
    s.hardware_queues = hardwareQueues();
    s.collapse_wanted = collapse_wanted;
    return s;
}

}  // namespace rpvg_hip_detail

namespace {

static_assert(kEmSideStreams == rpvg_hip_ctx::kAuxStreams && kEmCollapseMaxProblems + 2 == kCollapseMaxMatrices, "em_plan.hpp restates these");

// the scratch of the counting launches: per segment what it keeps, per problem the read mass of its rows without a selected path
struct EmCountBuffers {
    DeviceBuffer<uint32_t> * seg_rows, * seg_entries;
    DeviceBuffer<double> * seg_zero, * seg_total;
};

// The count-only half of the fill: fillSegmentsKernel<false> and fillOffsetsKernel on `view` — with storage in it the problems'
// terminal offsets and size bins too.  Returns the launches' arguments in `fa` for the launches that write.
int queueEmCount(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const EmProblemList & list, const EmOutputs & out, const EmProblemsView & view,
                 const EmCountBuffers & buffers, const EmBinRule rule, EmQueues * queues, uint32_t * prob_bucket, const EmFillPlan & plan, FillArgs & fa) {
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(buffers.seg_rows->alloc(list.items_bound));
    RPVG_HIP_CHECK(buffers.seg_entries->alloc(list.items_bound));
    RPVG_HIP_CHECK(buffers.seg_zero->alloc(list.items_bound));
    RPVG_HIP_CHECK(buffers.seg_total->alloc(list.items_bound));
    fa = FillArgs{};
    fa.num_problems = list.P_bound;
    fa.num_problems_dev = list.d_num_problems;
    fa.num_items = list.items_bound;
    fa.num_items_dev = list.d_num_items;
    fa.seg_first = list.d_seg_first;
    fa.item_problem = list.d_item_problem;
    fa.prob_cluster = list.d_cluster;
    fa.col_path = list.d_col_path;
    fa.cluster_row_off = batch->cluster_row_off.ptr;
    fa.cluster_path_off = batch->cluster_path_off.ptr;
    fa.row_ent_off = batch->row_ent_off.ptr;
    fa.ent_path = batch->ent_path.ptr;
    fa.ent_prob = batch->ent_prob.ptr;
    fa.row_count = batch->row_count.ptr;
    fa.row_noise = batch->row_noise.ptr;
    fa.problems = view;
    fa.seg_rows = buffers.seg_rows->ptr;
    fa.seg_entries = buffers.seg_entries->ptr;
    fa.seg_zero_mass = buffers.seg_zero->ptr;
    fa.seg_total_mass = buffers.seg_total->ptr;
    fa.kept_entries = out.d_kept_entries;
    fa.prob_bucket = prob_bucket;
    fa.queues = queues;
    fa.rule = rule;
    fa.lds_map_paths = plan.lds_map_paths;
    fa.long_row_scratch = plan.long_row_scratch ? 1u : 0u;
    fa.num_fused = 0;
    RPVG_HIP_CHECK(launchFillSegments<false>(fa, plan, st));
    fillOffsetsKernel<<<dim3((list.P_bound + 255) / 256), dim3(256), 0, st>>>(fa);
    return RPVG_HIP_OK;
}

// The fused build: a problem of the grid bin that will be solved on a dense matrix (em_grid.hip) gets it from the compaction
// itself — rows -> matrix, 12 B read per entry and 8 B written per cell, against rows -> CSR -> zeroed matrix -> matrix (the
// 1 M x 2 000 cluster of BASELINE.json configs[1]: 36 ms of a 160 ms call).  The host has to see the counts for it (one small
// copy and its wait, only in a solve that sits on a cluster large enough for the grid bin: EmSolvePlan::fused_look).
// RPVG_HIP_NO_FUSED_DENSE=1: never.
int lookForFusedDense(rpvg_hip_ctx * ctx, const uint32_t P, EmSolveWork & work, FillArgs & fa) {
    hipStream_t st = ctx->stream;
    DeviceBuffer<DenseCandidates> d_candidates;
    DenseCandidates * h_candidates = nullptr;
    RPVG_HIP_CHECK(d_candidates.alloc(1));
    if (pinnedAlloc(reinterpret_cast<void **>(&h_candidates), sizeof(DenseCandidates)) != hipSuccess) {
        setError("rpvg_hip_em_solve: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    struct PinnedGuard {
        void * p;
        ~PinnedGuard() { pinnedFree(p); }
    } pinned_guard{h_candidates};
    RPVG_HIP_CHECK(zeroAsync(d_candidates.ptr, sizeof(DenseCandidates), st));
    denseCandidatesKernel<<<dim3((P + 255) / 256), dim3(256), 0, st>>>(fa, d_candidates.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipMemcpyAsync(h_candidates, d_candidates.ptr, sizeof(DenseCandidates), hipMemcpyDeviceToHost, st));
    {
        HostScope wait_scope("em_solve: the counts of the large problems");
        RPVG_HIP_CHECK(waitStream(st));
    }
    const uint32_t n = std::min<uint32_t>(h_candidates->count, kEmMaxFusedDense);
    for (uint32_t i = 0; i < n; ++i) {
        const DenseCandidate & c = h_candidates->list[i];
        if (!emGridDenseRoute(c.columns, c.rows, c.entries)) continue;
        const uint64_t ld = (static_cast<uint64_t>(c.columns) + 1) & ~1ull;
        DeviceBuffer<double> & m = work.fused_matrix[work.num_fused];
        // (without the memory for it the problem takes the CSR, and the grid route decides again)
        if (m.alloc(static_cast<size_t>(c.rows) * ld) != hipSuccess) {
            (void) hipGetLastError();
            continue;
        }
        work.fused[work.num_fused] = EmFusedDense{c.problem, 0u, m.ptr, ld};
        fa.fused[work.num_fused] = work.fused[work.num_fused];
        ++work.num_fused;
    }
    fa.num_fused = work.num_fused;
    return RPVG_HIP_OK;
}

EmQueues * queuesOf(const EmSolveWork & work) { return reinterpret_cast<EmQueues *>(work.zeroed_queues ? work.zeroed_queues : work.d_queues.ptr); }

}  // namespace

namespace rpvg_hip_detail {

// Stage 1: allocations, the three fill launches (four with fused dense matrices) and the look between them.  Caller holds
// ctx->mutex and has set the device; `work` must outlive the kernels.  build_span: the FAM_BUILD span, opened behind the
// allocations; the caller closes it (a solve: behind emOrderKernel).
int queueEmFill(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const EmProblemList & list, const EmOutputs & out, EmSolveWork & work,
                const EmSolveKnobs & knobs, const EmFillPlan & plan, const bool fused_look, int & build_span) {
    hipStream_t st = ctx->stream;
    const uint32_t P = list.P_bound;
    RPVG_HIP_CHECK(work.d_prow_off.alloc(list.rows_capacity + P));
    RPVG_HIP_CHECK(work.d_prow_count.alloc(list.rows_capacity));
    RPVG_HIP_CHECK(work.d_prow_noise.alloc(list.rows_capacity));
    RPVG_HIP_CHECK(work.d_pent_col.alloc(list.entries_capacity));
    RPVG_HIP_CHECK(work.d_pent_val.alloc(list.entries_capacity));
    RPVG_HIP_CHECK(work.d_zero.alloc(P));
    RPVG_HIP_CHECK(work.d_bucket.alloc(P));
    RPVG_HIP_CHECK(work.d_order.alloc(P));
    if (!work.zeroed_queues) RPVG_HIP_CHECK(work.d_queues.alloc(sizeof(EmQueues)));
    if (list.wide_capacity > 0) {
        RPVG_HIP_CHECK(work.d_wide_vectors.alloc(list.wide_capacity));
        RPVG_HIP_CHECK(work.d_wide_off.alloc(P));
    }
    build_span = ctx->spanBegin(FAM_BUILD);
    if (!work.zeroed_queues) RPVG_HIP_CHECK(zeroAsync(work.d_queues.ptr, sizeof(EmQueues), st));
    FillArgs fa;
    const EmCountBuffers buffers{&work.d_seg_rows, &work.d_seg_entries, &work.d_seg_zero, &work.d_seg_total};
    const int rc = queueEmCount(ctx, batch, list, out, work.view(list, out), buffers, knobs.rule, queuesOf(work), work.d_bucket.ptr, plan, fa);
    if (rc != RPVG_HIP_OK) return rc;
    if (fused_look) {
        const int look = lookForFusedDense(ctx, P, work, fa);
        if (look != RPVG_HIP_OK) return look;
    }
    RPVG_HIP_CHECK(launchFillSegments<true>(fa, plan, st));
    if (fa.num_fused > 0) {
        uint64_t widest = 0;
        for (uint32_t f = 0; f < fa.num_fused; ++f) widest = std::max(widest, fa.fused[f].ld);
        const size_t lds = emFillDenseLdsBytes(fa.lds_map_paths, widest);
        if (lds > kLdsOptIn) RPVG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&fillDenseRowsKernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        fillDenseRowsKernel<<<dim3(plan.dense_grid, fa.num_fused), dim3(256), lds, st>>>(fa);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
    }
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 3;
    return RPVG_HIP_OK;
}

}  // namespace rpvg_hip_detail

namespace {

// Stage 2: readCollapseProbabilityMatrix on the rows of every problem (src/path_abundance_estimator.cpp:266,668), on the collapse
// stream behind the fill (work.filled); the EM kernels wait for it and read the merged counts of the problems it merged rows in
// (EmProblemsView::mergedRows).  (A first version solved every problem next to the collapse and the merged ones a second time: on
// the configs[2] batch the largest problems were the merged ones, the second pass took as long as the first, and the collapse's
// forty launches took 2.6 ms in between the persistent EM kernels against 1.5 ms without them.)
int queueEmCollapse(rpvg_hip_ctx * ctx, const EmProblemList & list, const EmSolvePlan & plan, const EmSolveKnobs & knobs, const double precision,
                    EmSolveWork & work, EmProblemsView & view, std::unique_ptr<HostScope> & stage_scope) {
    auto cw = std::make_shared<CsrCollapseWork>();
    work.collapse = cw;
    RPVG_HIP_CHECK(hipEventCreateWithFlags(&work.collapsed, hipEventDisableTiming));
    RPVG_HIP_CHECK(hipStreamWaitEvent(ctx->collapse_stream, work.filled, 0));
    CsrCollapseInput in;
    in.num_problems_bound = list.P_bound;
    in.num_problems_dev = list.d_num_problems;
    in.rows_capacity = list.rows_capacity;
    in.problems = view;
    in.num_items_bound = list.items_bound;
    in.num_items_dev = list.d_num_items;
    in.seg_first = list.d_seg_first;
    in.item_problem = list.d_item_problem;
    in.segment_rows = kFillSegmentRows;
    in.max_rows_bound = plan.collapse_max_rows;
    const int collapse_span = ctx->spanBegin(FAM_COLLAPSE, ctx->collapse_stream);
    RPVG_HIP_CHECK(hipEventCreateWithFlags(&work.collapse_sorted, hipEventDisableTiming));
    stage_scope.reset(new HostScope("em_solve: the problems' collapse queued"));
    RPVG_HIP_CHECK(queueCsrCollapse(ctx, in, precision, *cw, ctx->collapse_stream, work.collapse_sorted));
    stage_scope.reset(new HostScope("em_solve: EM launches, grid problems, join"));
    ctx->spanEnd(collapse_span);
    RPVG_HIP_CHECK(hipEventRecord(work.collapsed, ctx->collapse_stream));
    view.merged_count = cw->merged_count.ptr;
    view.problem_merged = cw->problem_merged.ptr;
    RPVG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, work.collapsed, 0));
    // The EM launches go to streams of their own, and a stream whose next command waits for an event holds its hardware
    // queue meanwhile — eight queues for every stream of both lanes (hardwareQueues()).  Queued at once, ten launches that
    // wait for the collapse parked most of the queues for its whole millisecond and the other lane's kernels stood behind
    // them (measured: the library's segmented sort, whose host wait for its partition sizes delayed these launches by
    // accident, beat every sort without such a wait by 1 ms per batch).  So the submitting thread waits for the collapse
    // itself and queues the launches then.
    // RPVG_HIP_EM_LAUNCH_EARLY=1: queue them at once (A/B).
    if (!knobs.launch_early && work.collapse_sorted) {
        HostScope wait_scope("em_solve: wait for the collapse");
        RPVG_HIP_CHECK(waitEvent(knobs.wait_sort_only ? work.collapse_sorted : work.collapsed));
    }
    return RPVG_HIP_OK;
}

// Stage 3: the plan's table, one persistent launch per row (the side streams are joined behind the problems that run over the
// whole GPU: those start while these kernels run).  Every launch carries its own HIP events on its own stream
// (rpvg_hip_kernel_stats::em_kernel).
int queueEmLaunches(rpvg_hip_ctx * ctx, const EmSolvePlan & plan, EmLaunchArgs & args) {
    RPVG_HIP_CHECK(ctx->forkAux());
    for (int i = 0; i < plan.num_launches; ++i) {
        const EmLaunch & l = plan.launches[i];
        hipStream_t on = l.stream == kEmMainStream ? ctx->stream : ctx->aux[l.stream];
        args.bin = l.bin;
        const int bin_span = ctx->spanBegin(FAM_EM_KERNEL, on, static_cast<int>(l.bin));
        hipError_t e = hipSuccess;
        switch (l.variant) {
            case EmVariant::kSparse64Resident: e = launchEm<64, true>(args, l.grid, l.lds, on); break;
            case EmVariant::kSparse256Resident: e = launchEm<256, true>(args, l.grid, l.lds, on); break;
            case EmVariant::kSparse1024Resident: e = launchEm<1024, true>(args, l.grid, l.lds, on); break;
            case EmVariant::kSparse256Streamed: e = launchEm<256, false>(args, l.grid, l.lds, on); break;
            case EmVariant::kSparse1024Streamed: e = launchEm<1024, false>(args, l.grid, l.lds, on); break;
            case EmVariant::kSparseWide: e = launchEm<1024, false, true>(args, l.grid, l.lds, on); break;
            case EmVariant::kRegisterBins:
            case EmVariant::kWaveBins: e = launchEmRegisterBins(args, emLaunchRoles(plan, l), l.lds, on); break;
            case EmVariant::kSparse1024Bins:
                e = plan.wide_possible ? launchEmRoles<true>(args, emLaunchRoles(plan, l), l.lds, on) : launchEmRoles<false>(args, emLaunchRoles(plan, l), l.lds, on);
                break;
            case EmVariant::kRegister1x16: e = launchEmRegister<1, 16>(args, l.grid, l.lds, on); break;
            case EmVariant::kRegister2x16: e = launchEmRegister<2, 16>(args, l.grid, l.lds, on); break;
            case EmVariant::kRegister4x16: e = launchEmRegister<4, 16>(args, l.grid, l.lds, on); break;
            case EmVariant::kRegister1x32: e = launchEmRegister<1, 32>(args, l.grid, l.lds, on); break;
            case EmVariant::kRegister2x32: e = launchEmRegister<2, 32>(args, l.grid, l.lds, on); break;
        }
        RPVG_HIP_CHECK(e);
        ctx->spanEnd(bin_span);
    }
    return RPVG_HIP_OK;
}

// Stage 4, first half (in front of the EM launches on the context's stream): the problems of the grid bin described for the host
struct EmGridLook {
    DeviceBuffer<EmGridProblem> d_problems;
    hipEvent_t described = nullptr;
    uint32_t * h_count = nullptr;   // pinned
    ~EmGridLook() {
        if (described) (void) hipEventDestroy(described);
        if (h_count) pinnedFree(h_count);
    }
};
int queueEmGridLook(rpvg_hip_ctx * ctx, const uint32_t P, const EmProblemsView & view, const EmOutputs & out, const EmSolveWork & work, EmGridLook & look) {
    hipStream_t st = ctx->stream;
    EmQueues * queues = queuesOf(work);
    RPVG_HIP_CHECK(look.d_problems.alloc(P));
    if (pinnedAlloc(reinterpret_cast<void **>(&look.h_count), 64) != hipSuccess) {
        setError("rpvg_hip_em_solve: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    GridDescribeArgs da;
    da.queues = queues;
    da.order = work.d_order.ptr;
    da.problems = view;
    da.kept_entries = out.d_kept_entries;
    da.out = look.d_problems.ptr;
    da.capacity = P;
    emGridDescribeKernel<<<dim3((P + 255) / 256), dim3(256), 0, st>>>(da);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipMemcpyAsync(look.h_count, &queues->bin_count[kEmGridBin], sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipEventCreateWithFlags(&look.described, hipEventDisableTiming));
    RPVG_HIP_CHECK(hipEventRecord(look.described, st));
    return RPVG_HIP_OK;
}

// Stage 4, second half (behind the EM launches): the described problems solved over the whole GPU while the one-workgroup kernels
// run, then the join of the side streams
int queueEmGridAndJoin(rpvg_hip_ctx * ctx, const uint32_t P, const EmProblemsView & view, const EmOutputs & out, const EmSolveWork & work,
                       const EmSolveKnobs & knobs, EmGridLook * look, const uint32_t max_em_its, const double max_rel_em_conv) {
    hipStream_t st = ctx->stream;
    if (look) {
        RPVG_HIP_CHECK(waitEvent(look->described));
        const uint32_t n_grid = std::min<uint32_t>(*look->h_count, P);
        if (n_grid > 0) {
            std::vector<EmGridProblem> grid_problems(n_grid);
            RPVG_HIP_CHECK(hipMemcpyAsync(grid_problems.data(), look->d_problems.ptr, sizeof(EmGridProblem) * n_grid, hipMemcpyDeviceToHost, st));
            RPVG_HIP_CHECK(waitStream(st));
            EmGridStorage storage;
            storage.problems = view;
            storage.abundances = out.d_abundances;
            storage.noise_count = out.d_noise_count;
            storage.iterations = out.d_iterations;
            storage.fused = work.fused;
            storage.num_fused = work.num_fused;
            const int rc = runEmGridProblems(ctx, st, grid_problems.data(), n_grid, storage, max_em_its, max_rel_em_conv);
            if (rc != RPVG_HIP_OK) return rc;
        }
    }
    // (RPVG_HIP_EM_JOIN_ON_STREAM=1: the context's stream waits for the side streams, not the thread — A/B)
    RPVG_HIP_CHECK(knobs.join_on_stream ? ctx->joinAux() : ctx->joinAuxOnHost());
    return RPVG_HIP_OK;
}

// RPVG_HIP_EM_COLLAPSE_DEBUG: what the collapse of a solve did (synchronises: a measuring aid)
int dumpEmCollapse(rpvg_hip_ctx * ctx, const EmProblemList & list, const EmSolveWork & work) {
    const CsrCollapseWork * cw = static_cast<const CsrCollapseWork *>(work.collapse.get());
    const uint32_t P = list.P_bound;
    using namespace rpvg_collapse;
    const InfoLayout layout = infoLayout(P, list.rows_capacity);
    uint32_t info[kInfoWords] = {0}, merged = 0, problems = P, counts[3] = {0};  // counts: the marked list, the forward pairs, the around pairs
    RPVG_HIP_CHECK(waitStream(ctx->stream));
    RPVG_HIP_CHECK(hipMemcpy(info, cw->info.ptr + layout.info, sizeof(info), hipMemcpyDeviceToHost));
    RPVG_HIP_CHECK(hipMemcpy(&merged, cw->problem_merged.ptr + P, sizeof(merged), hipMemcpyDeviceToHost));
    if (list.d_num_problems) RPVG_HIP_CHECK(hipMemcpy(&problems, list.d_num_problems, sizeof(problems), hipMemcpyDeviceToHost));
    RPVG_HIP_CHECK(hipMemcpy(counts, cw->info.ptr + layout.marked_count, sizeof(counts), hipMemcpyDeviceToHost));  // (marked_count, pair_counts[2]: side by side)
    std::fprintf(stderr, "[em collapse] marked rows %u forward pairs %u (equal up to rounding %u, apart %u) around pairs %u\n", counts[0], counts[1],
                 info[kInfoPairsEquivalent], info[kInfoPairsApart], counts[2]);
    std::fprintf(stderr, "[em collapse] problems %u (bound %u) row slots %llu: replayed %u whole %u active rows %u rows replaced %u problems merged %u\n", problems, P,
                 static_cast<unsigned long long>(list.rows_capacity), info[kInfoMatrices], info[kInfoWholeMatrices], info[kInfoActiveRows], info[kInfoRowsReplaced], merged);
    return RPVG_HIP_OK;
}

}  // namespace

namespace rpvg_hip_detail {

// The stages above in order, queued on the context's streams without a host synchronisation of its own but for the looks the
// plan asks for.  Caller holds ctx->mutex and has set the device; `work` must outlive the kernels.
int queueEmSolve(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const EmProblemList & list, const uint32_t max_em_its,
                 const double max_rel_em_conv, const EmOutputs & out, EmSolveWork & work, const double collapse_precision) {
    hipStream_t st = ctx->stream;
    const uint32_t P = list.P_bound;
    const EmSolveKnobs knobs = emSolveKnobs();
    const EmSolvePlan plan = planEmSolve(emSolveShape(ctx, list, collapse_precision > 0), knobs);
    std::unique_ptr<HostScope> stage_scope(new HostScope("em_solve: allocations + fill queued"));
    int span = -1;
    int rc = queueEmFill(ctx, batch, list, out, work, knobs, plan.fill, plan.fused_look, span);
    if (rc != RPVG_HIP_OK) return rc;
    // (a solve that is too large for the collapse gets an error rather than results without it)
    RPVG_REQUIRE(!plan.collapse_too_large,
                 "EM solve with a row collapse: %llu row slots in %u problems exceed what one solve can collapse (2^31 - 1 rows, 2^20 - 2 problems): split the problem list",
                 static_cast<unsigned long long>(list.rows_capacity), P);
    if (plan.collapse) {
        RPVG_HIP_CHECK(hipEventCreateWithFlags(&work.filled, hipEventDisableTiming));
        RPVG_HIP_CHECK(hipEventRecord(work.filled, st));
    }
    emOrderKernel<<<dim3((P + 255) / 256), dim3(256), 0, st>>>(P, list.d_num_problems, work.d_bucket.ptr, list.d_col_off, queuesOf(work), work.d_order.ptr,
                                                              work.d_wide_off.ptr, list.wide_capacity, plan.mid_grid_allowed ? 1u : 0u);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->spanEnd(span);
    ctx->stats.build_launches += 1;

    EmProblemsView view = work.view(list, out);
    if (plan.collapse) {
        rc = queueEmCollapse(ctx, list, plan, knobs, collapse_precision, work, view, stage_scope);
        if (rc != RPVG_HIP_OK) return rc;
    }

    EmLaunchArgs args;
    args.order = work.d_order.ptr;
    args.queues = queuesOf(work);
    args.bin = 0;
    args.problems = view;
    args.max_em_its = max_em_its;
    args.register_copies = knobs.register_copies ? 1u : 0u;
    args.max_rel_em_conv = max_rel_em_conv;
    args.wide_vectors = work.d_wide_vectors.ptr;
    args.wide_off = work.d_wide_off.ptr;
    args.wide_capacity = list.wide_capacity;
    args.abundances = out.d_abundances;
    args.noise_count = out.d_noise_count;
    args.iterations = out.d_iterations;

    EmGridLook look;
    if (plan.grid_possible) {
        rc = queueEmGridLook(ctx, P, view, out, work, look);
        if (rc != RPVG_HIP_OK) return rc;
    }
    span = ctx->spanBegin(FAM_EM_SPARSE);
    rc = queueEmLaunches(ctx, plan, args);
    if (rc != RPVG_HIP_OK) return rc;
    rc = queueEmGridAndJoin(ctx, P, view, out, work, knobs, plan.grid_possible ? &look : nullptr, max_em_its, max_rel_em_conv);
    if (rc != RPVG_HIP_OK) return rc;
    ctx->spanEnd(span);  // (behind the join: the span of the solve's kernels on all of its streams)
    if (plan.collapse && knobs.collapse_debug) return dumpEmCollapse(ctx, list, work);
    return RPVG_HIP_OK;
}

// Folds the results of a solve into the context's statistics (after the results have reached the host): the host
// repeats the device's bin decision per problem.  cols[p] = columns of problem p without the noise component.
void accountEmSolve(rpvg_hip_ctx * ctx, const uint32_t P, const uint64_t * col_off, const uint32_t * kept_rows, const uint32_t * kept_entries,
                    const uint32_t * iterations) {
    // algorithmic bytes: per iteration 12 B per entry (value + column), 20 B per row (count, noise, offset), 16 B per
    // column (a read + a' write)
    const EmSolveKnobs knobs = emSolveKnobs();
    const EmBinRule rule = knobs.rule;
    double bin_bytes[kEmBins] = {};
    uint64_t bin_its[kEmBins] = {}, bin_problems[kEmBins] = {};
    uint32_t bin_slowest[kEmBins] = {};
    // (emOrderKernel's verdict on the few mid-size problems, from the same rule)
    uint32_t mid_problems = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t C = static_cast<uint32_t>(col_off[p + 1] - col_off[p]) + 1;
        if (emIsMidSize(static_cast<uint32_t>(emBinOf(rule, C, kept_rows[p], kept_entries[p])), emWorkBucket(kept_rows[p], kept_entries[p]))) ++mid_problems;
    }
    const bool mid_moved = emMidGridMoves(emMidGridAllowed(rule.grid_min_work), mid_problems);
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t C = static_cast<uint32_t>(col_off[p + 1] - col_off[p]) + 1;
        const int b = emRouteOf(emBinOf(rule, C, kept_rows[p], kept_entries[p]), emWorkBucket(kept_rows[p], kept_entries[p]), mid_moved);
        // (a problem of the grid bin on the dense route ran em_dense.hip's kernels: emDenseIterate has accounted for it)
        if (b == kEmGridBin && emGridDenseRoute(C, kept_rows[p], kept_entries[p])) {
            bin_problems[b] += 1;
            continue;
        }
        bin_bytes[b] += static_cast<double>(iterations[p]) * (12.0 * kept_entries[p] + 20.0 * kept_rows[p] + 16.0 * C);
        bin_its[b] += iterations[p];
        bin_problems[b] += 1;
        bin_slowest[b] = std::max(bin_slowest[b], iterations[p]);
    }
    double slot_bytes[kEmBins] = {};
    uint64_t slot_its[kEmBins] = {}, slot_problems[kEmBins] = {};
    uint32_t slot_slowest[kEmBins] = {};
    for (int b = 0; b < kEmBins; ++b) {
        const int slot = emStatsSlot(b, knobs.one_register_launch);
        slot_bytes[slot] += bin_bytes[b];
        slot_its[slot] += bin_its[b];
        slot_problems[slot] += bin_problems[b];
        slot_slowest[slot] = std::max(slot_slowest[slot], bin_slowest[b]);
    }
    for (int b = 0; b < kEmBins; ++b) {
        if (!slot_problems[b]) continue;
        rpvg_hip_em_kernel_stats & ks = ctx->stats.em_kernel[b];
        ks.launches += 1;
        ks.problems += slot_problems[b];
        ks.iterations += slot_its[b];
        ks.max_iterations += slot_slowest[b];
        ks.alg_bytes += slot_bytes[b];
        ctx->stats.em_sparse_launches += 1;
        ctx->stats.em_sparse_alg_bytes += slot_bytes[b];
        ctx->stats.em_iterations_total += slot_its[b];
    }
}

namespace {
// Free device memory a call may plan with (a share of what the driver reported when the process first asked: other lanes
// allocate too, and hipMemGetInfo costs milliseconds — asked per call it was 3 ms of every batch's critical path).
uint64_t deviceMemoryBudget() {
    static const uint64_t budget = []() {
        size_t free_bytes = 0, total_bytes = 0;
        if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) {
            (void) hipGetLastError();
            return static_cast<uint64_t>(4ull << 30);
        }
        return static_cast<uint64_t>(free_bytes) * 2 / 5;
    }();
    return budget;
}
}  // namespace

int prepareHostProblems(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_em_problems * problems,
                        HostProblemSet & ps, const EmOutputs & out, const char * who) {
    const uint32_t P = problems->num_problems;
    std::unique_ptr<HostScope> scope(new HostScope("problems: validate"));
    std::vector<uint64_t> row_base(P), ent_base(P), cluster_rows(P), cluster_entries(P);
    EmProblemList & list = ps.list;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t k = problems->cluster[p];
        RPVG_REQUIRE(k < batch->num_clusters, "%s: problem %u refers to cluster %u of %u", who, p, k, batch->num_clusters);
        const uint64_t n_paths = batch->h_cluster_path_off[k + 1] - batch->h_cluster_path_off[k];
        const uint64_t c0 = problems->col_off[p], c1 = problems->col_off[p + 1];
        RPVG_REQUIRE(c1 > c0, "%s: problem %u has no columns", who, p);
        RPVG_REQUIRE(batch->h_cluster_row_off[k + 1] > batch->h_cluster_row_off[k], "%s: problem %u is on cluster %u which has no rows", who, p, k);
        for (uint64_t c = c0; c < c1; ++c) {
            RPVG_REQUIRE(problems->col_path[c] < n_paths, "%s: problem %u column path %u >= %llu", who, p, problems->col_path[c],
                         static_cast<unsigned long long>(n_paths));
            RPVG_REQUIRE(c == c0 || problems->col_path[c] > problems->col_path[c - 1], "%s: problem %u columns are not strictly ascending", who, p);
        }
        const uint32_t C = static_cast<uint32_t>(c1 - c0) + 1;
        cluster_rows[p] = batch->h_cluster_row_off[k + 1] - batch->h_cluster_row_off[k];
        cluster_entries[p] = batch->h_cluster_ent_off[k + 1] - batch->h_cluster_ent_off[k];
        list.max_cols = std::max<uint32_t>(list.max_cols, C);
        list.max_cluster_paths = std::max<uint32_t>(list.max_cluster_paths, static_cast<uint32_t>(n_paths));
        list.max_cluster_work = std::max<uint64_t>(list.max_cluster_work, cluster_rows[p] + cluster_entries[p]);
        if (emLdsBytes(C, 0, 0, 256, false) > kEmLdsLimit) list.wide_capacity += 2ull * C;
    }
    uint64_t rows_bound = 0, entries_bound = 0;
    emStorageBases(cluster_rows.data(), cluster_entries.data(), P, row_base.data(), ent_base.data(), &rows_bound, &entries_bound);
    ps.n_cols_total = problems->col_off[P];
    list.P_bound = P;
    // work items of the compaction: the rows of every problem's cluster in segments
    std::vector<uint64_t> seg_first(P + 1, 0);
    for (uint32_t p = 0; p < P; ++p) seg_first[p + 1] = seg_first[p] + (cluster_rows[p] + kFillSegmentRows - 1) / kFillSegmentRows;
    RPVG_REQUIRE(seg_first[P] < 0xffffffffull, "%s: too many row segments (%llu)", who, static_cast<unsigned long long>(seg_first[P]));
    std::vector<uint32_t> item_problem(seg_first[P]);
    for (uint32_t p = 0; p < P; ++p) {
        for (uint64_t item = seg_first[p]; item < seg_first[p + 1]; ++item) item_problem[item] = p;
    }
    list.items_bound = static_cast<uint32_t>(seg_first[P]);

    scope.reset(new HostScope("problems: uploads"));
    hipStream_t st = ctx->stream;
    const EmSolveKnobs knobs = emSolveKnobs();
    const uint64_t bound_budget = knobs.has_bound_bytes ? knobs.bound_bytes : std::min<uint64_t>(32ull << 30, deviceMemoryBudget());
    const bool by_bound = emStorageByBound(rows_bound, entries_bound, bound_budget);
    int span = ctx->spanBegin(FAM_H2D);
    ps.uploads.add(ps.d_cluster, problems->cluster, P);
    ps.uploads.add(ps.d_col_off, problems->col_off, P + 1);
    ps.uploads.add(ps.d_col_path, problems->col_path, ps.n_cols_total);
    ps.uploads.add(ps.d_seg_first, seg_first.data(), P + 1);
    ps.uploads.add(ps.d_item_problem, item_problem.data(), item_problem.size());
    if (by_bound) {
        ps.uploads.add(ps.d_row_base, row_base.data(), P);
        ps.uploads.add(ps.d_ent_base, ent_base.data(), P);
    }
    RPVG_HIP_CHECK(ps.uploads.commit(st));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(P * 4 + (P + 1) * 24 + ps.n_cols_total * 4);
    list.d_cluster = ps.d_cluster.ptr;
    list.d_col_off = ps.d_col_off.ptr;
    list.d_col_path = ps.d_col_path.ptr;
    list.d_seg_first = ps.d_seg_first.ptr;
    list.d_item_problem = ps.d_item_problem.ptr;
    if (!by_bound) {
        scope.reset(new HostScope("problems: counting pass"));
        // counts only: no storage, no queues (the view of a solve's work without buffers)
        EmSolveWork count_work;
        RPVG_HIP_CHECK(count_work.d_zero.alloc(P));
        const EmCountBuffers buffers{&count_work.d_seg_rows, &count_work.d_seg_entries, &count_work.d_seg_zero, &count_work.d_seg_total};
        FillArgs fa;
        const int rc = queueEmCount(ctx, batch, list, out, count_work.view(list, out), buffers, knobs.rule, nullptr, nullptr, planEmFill(emSolveShape(ctx, list, false), knobs), fa);
        if (rc != RPVG_HIP_OK) return rc;
        RPVG_HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> kept_rows(P), kept_ent(P);
        RPVG_HIP_CHECK(hipMemcpyAsync(kept_rows.data(), out.d_kept_rows, P * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipMemcpyAsync(kept_ent.data(), out.d_kept_entries, P * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(waitStream(st));
        emStorageBases(kept_rows.data(), kept_ent.data(), P, row_base.data(), ent_base.data(), &rows_bound, &entries_bound);
        RPVG_HIP_CHECK(ps.d_row_base.upload(row_base.data(), P, st));
        RPVG_HIP_CHECK(ps.d_ent_base.upload(ent_base.data(), P, st));
    }
    list.d_row_base = ps.d_row_base.ptr;
    list.d_ent_base = ps.d_ent_base.ptr;
    list.rows_capacity = rows_bound;
    list.entries_capacity = entries_bound;
    return RPVG_HIP_OK;
}

}  // namespace rpvg_hip_detail

extern "C" const char * rpvg_hip_em_kernel_name(int index) {
    // (the size bins of rpvg_hip_em_solve, in bin order)
    // (emRegisterKernel: the five register-resident bins — <1,16> <2,16> <4,16> <1,32> <2,32> — in one launch, under the first
    // one's index; with RPVG_HIP_EM_REGISTER_LAUNCHES=5 every bin has its own launch of emRegisterBinKernel and its own index)
    // (merged launches — the bins of 64 and of 1 024 threads — keep the names: a slot's problems and iterations are its bin's, and
    // the device time of a launch stands under one of its bins' slots, 4 and 7: docs/design/kernels-em.md)
    static const char * const names[RPVG_HIP_EM_KERNELS] = {
        "emSparseKernel<64,true>", "emSparseKernel<256,true>", "emSparseKernel<256,false>", "emSparseKernel<1024,false>",
        "emRegisterBinKernel<1,16>", "emRegisterBinKernel<2,16>", "emRegisterBinKernel<4,16>", "emSparseKernel<1024,true>",
        "emRegisterBinKernel<1,32>", "emRegisterBinKernel<2,32>", "emSparseKernel<1024,false,WIDE>", "emGridAccumKernel"};
    if (index < 0 || index >= RPVG_HIP_EM_KERNELS) return nullptr;
    // (the slot that stands for all register bins is the launch of all of them)
    if (index == static_cast<int>(kRegisterKernelIndex) && emStatsSlot(static_cast<int>(kRegisterBins[0]), emSolveKnobs().one_register_launch) == index) return "emRegisterKernel";
    return names[index];
}

extern "C" int rpvg_hip_em_solve(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t max_em_its,
                                 double max_rel_em_conv, const rpvg_hip_em_problems * problems,
                                 rpvg_hip_em_results * results) {
    RPVG_REQUIRE(ctx && batch && problems && results, "rpvg_hip_em_solve: NULL argument");
    const uint32_t P = problems->num_problems;
    if (P == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(problems->cluster && problems->col_off && problems->col_path, "rpvg_hip_em_solve: NULL problem arrays");
    RPVG_REQUIRE(results->abundances && results->noise_count && results->total_count && results->iterations,
                 "rpvg_hip_em_solve: NULL result arrays");
    RPVG_REQUIRE(max_em_its > 0, "rpvg_hip_em_solve: max_em_its must be positive");

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // the results and the per-problem counts in one block, one copy back
    std::vector<uint32_t> kept_rows(P), kept_ent(P);
    DeviceBuffer<uint32_t> d_iters, d_kept_rows, d_kept_ent;
    DeviceBuffer<double> d_abund, d_noise_count, d_total;
    DownloadPack outputs;
    outputs.add(d_abund, results->abundances, problems->col_off[P]);
    outputs.add(d_noise_count, results->noise_count, P);
    outputs.add(d_total, results->total_count, P);
    outputs.add(d_iters, results->iterations, P);
    outputs.add(d_kept_rows, kept_rows.data(), P);
    outputs.add(d_kept_ent, kept_ent.data(), P);
    RPVG_HIP_CHECK(outputs.alloc());
    EmOutputs out{d_abund.ptr, d_noise_count.ptr, d_iters.ptr, d_kept_rows.ptr, d_kept_ent.ptr, d_total.ptr};

    HostProblemSet ps;
    int rc = prepareHostProblems(ctx, batch, problems, ps, out, "rpvg_hip_em_solve");
    if (rc != RPVG_HIP_OK) return rc;
    std::unique_ptr<HostScope> scope(new HostScope("em_solve: launches"));
    rc = queueEmSolve(ctx, batch, ps.list, max_em_its, max_rel_em_conv, out, ps.work, problems->collapse_precision);
    if (rc != RPVG_HIP_OK) return rc;

    scope.reset(new HostScope("em_solve: wait for the kernels + download"));
    RPVG_HIP_CHECK(outputs.fetch(st));
    RPVG_HIP_CHECK(waitStream(st));
    outputs.scatter();
    scope.reset();
    accountEmSolve(ctx, P, problems->col_off, kept_rows.data(), kept_ent.data(), results->iterations);
    return RPVG_HIP_OK;
}

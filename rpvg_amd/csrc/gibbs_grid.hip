// Read-count Gibbs problems too wide or too large for one workgroup: every iteration runs over the whole GPU (gfx950).
//
// rpvg_hip_gibbs_read_counts puts every problem on ONE workgroup (gibbs_counts.hip, gibbsReadCountKernel): right for the
// thousands of small problems of a batch; a problem whose columns do not fit that kernel's LDS, or whose kept rows + entries
// reach gibbsGridMinWork() (em_grid.hip), comes here — the sampler's counterpart of em_grid.hip.  gibbsReadCountSampler
// (src/path_abundance_estimator.cpp:116-212) per Gibbs iteration: every row's reads are split multinomially over its columns
// with probabilities P_ij a_j / s_i (:149-178), every component draws Gamma(count_j + gamma, 1) and the vector is
// renormalised (:182-190), every `thin`-th state is recorded (:192-210).  Per iteration, queued without a host wait:
//
//   gibbsGridSplitKernel<LANES,LDS>  grid-wide pass over the problem's compacted CSR; a workgroup owns a contiguous range of
//                                    rows.  LANES = 1: a thread per row and the reference's chain of binomials (short rows).
//                                    LANES = 64: a wavefront per row, the lanes stride the row's entries, the row sum is a wave
//                                    reduction; a row of at most 64 reads draws them as categorical draws over the wave's
//                                    prefix sums, a row of more keeps the chain of binomials, every lane running the same
//                                    chain over the terms the wave computed.  Rows without a selected path put all their
//                                    reads on noise (the scalar Z the counts start from), the reads left after the last
//                                    entry go to noise.  LDS = true: abundances and counts of the workgroup in LDS, the
//                                    non-zero counts flushed with 64-bit integer atomics; false (a problem too wide): the
//                                    counts go straight to the global vector, the abundances come from global memory
//                                    (L2-resident at these sizes).  Counts are integers: no order of arrival changes a sum,
//                                    and there is no floating-point atomic anywhere.
//   gibbsGridUpdateKernel            g_j ~ Gamma(count_j + gamma, 1) per column, a partial sum per workgroup of 256 columns,
//                                    the counts reset for the next iteration (noise: Z).  The state is kept UNNORMALISED: the
//                                    probabilities of the split, P_ij g_j / sum_k P_ik g_k, do not change with the scale, and
//                                    whoever needs a_j = g_j / total adds the partial sums up in one fixed order (gridTotal).
//   gibbsGridRecordKernel            every `thin`-th iteration: a_j = g_j / total, min_gibbs_abundance applied as
//                                    gibbsReadCountKernel does, the sub-threshold mass as a partial sum per workgroup
//   gibbsGridNoiseKernel             once, at the end: the noise sample of every recorded state from those partial sums,
//                                    in workgroup order
//
// Launches, not a grid-wide barrier in a persistent kernel (em_grid.hip's header has the prices: ~1.5 us per dependent
// boundary against 4-7 us per barrier) — and a grid that is not fully resident cannot hang anything.
//
// Random numbers: Philox4x32-10 (gibbs_random.hpp) keyed by the problem's seed alone; the counter is
// (draw block, iteration, row or column, domain).  A problem's samples therefore depend on its seed and its data (which
// also choose the kernel variant) — not on the grid's size, the problem's position in the call or what else is in the batch.

#include "common.hpp"
#include "gibbs_random.hpp"

#include <algorithm>
#include <vector>

using namespace rpvg_hip_detail;

namespace {

constexpr double kMinGibbsAbundance = 1e-8;  // src/path_abundance_estimator.cpp:14
constexpr int kGibbsBlock = 256;
constexpr uint32_t kCategoricalMaxReads = 64;  // a lane per read
constexpr size_t kGibbsGridLdsLimit = 64 * 1024;  // abundances + counts of a workgroup, 16 B per column (two workgroups per CU and more)

// domains of the generator's counter
constexpr uint32_t kDomainRowChain = 0, kDomainRowCategorical = 1, kDomainColumn = 2;

__device__ __forceinline__ Philox gibbsGenerator(const uint64_t seed, const uint32_t domain, const uint32_t iteration, const uint32_t index) {
    Philox rng;
    rng.init(seed, domain, index);
    rng.ctr[1] = iteration;
    return rng;
}

// sum over the workgroup in one fixed order, in every thread (scratch: kGibbsBlock / 64 doubles)
__device__ __forceinline__ double gibbsBlockSum(double v, double * scratch) {
    v = waveSumF64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = scratch[0];
#pragma unroll
    for (int w = 1; w < kGibbsBlock / 64; ++w) total += scratch[w];
    return total;
}

// sum of the update kernel's partial sums: a function of their number alone
__device__ __forceinline__ double gridTotal(const double * partials, const uint32_t num_partials, double * scratch) {
    double local = 0.0;
    for (uint32_t b = threadIdx.x; b < num_partials; b += kGibbsBlock) local += partials[b];
    return gibbsBlockSum(local, scratch);
}

struct GibbsSplitArgs {
    uint32_t problem, C, rows, rows_per_block, iteration;
    uint64_t seed;
    // (the arrays of the EmProblemsView this kernel reads, member by member: with the view as one member the kernel's SGPR spills
    // moved; csrOf() below puts them back into a view)
    const uint64_t * row_base;
    const uint64_t * ent_base;
    const uint32_t * prow_off;
    const double * prow_count;
    const double * prow_noise;
    const uint32_t * pent_col;
    const double * pent_val;
    const double * g;                // [C] unnormalised abundances (last = noise)
    unsigned long long * counts;     // [C]
};

template <int LANES, bool LDS_COLS>
__global__ __launch_bounds__(kGibbsBlock) void gibbsGridSplitKernel(const GibbsSplitArgs args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gibbs_lds[];
    const uint32_t C = args.C, noise_col = C - 1;
    // LDS_COLS: [a: C doubles | counts: C words of 64 bits]; otherwise one word: the workgroup's reads on noise
    double * a_lds = reinterpret_cast<double *>(gibbs_lds);
    unsigned long long * c_lds = reinterpret_cast<unsigned long long *>(gibbs_lds) + (LDS_COLS ? C : 0);
    if (LDS_COLS) {
        for (uint32_t j = threadIdx.x; j < C; j += kGibbsBlock) {
            a_lds[j] = args.g[j];
            c_lds[j] = 0ull;
        }
    } else if (threadIdx.x == 0) {
        c_lds[0] = 0ull;
    }
    __syncthreads();
    const double * a = LDS_COLS ? a_lds : args.g;
    unsigned long long * counts = LDS_COLS ? c_lds : args.counts;
    unsigned long long * noise_word = LDS_COLS ? c_lds + noise_col : c_lds;

    const uint32_t p = args.problem;
    EmProblemsView view;
    view.prow_off = const_cast<uint32_t *>(args.prow_off);
    view.prow_count = const_cast<double *>(args.prow_count);
    view.prow_noise = const_cast<double *>(args.prow_noise);
    view.pent_col = const_cast<uint32_t *>(args.pent_col);
    view.pent_val = const_cast<double *>(args.pent_val);
    const EmProblemRows csr = view.at(p, args.row_base[p], args.ent_base[p], args.rows, false);
    const uint32_t * off = csr.off;
    const double * cnt = csr.count;
    const double * nzv = csr.noise;
    const uint32_t * col = csr.col;
    const double * val = csr.val;
    const uint32_t r0 = blockIdx.x * args.rows_per_block;
    const uint32_t r1 = min(args.rows, r0 + args.rows_per_block);
    const double a_noise = a[noise_col];
    unsigned long long to_noise = 0;

    if (LANES == 1) {
        // a thread per row: the loop of gibbsReadCountKernel (gibbs_counts.hip)
        for (uint32_t r = r0 + threadIdx.x; r < r1; r += kGibbsBlock) {
            const uint32_t e0 = off[r], e1 = off[r + 1];
            double s = nzv[r] * a_noise;
            for (uint32_t e = e0; e < e1; ++e) s += val[e] * a[col[e]];
            uint32_t remaining = static_cast<uint32_t>(cnt[r]);
            double remaining_prob = 1.0;
            Philox rng = gibbsGenerator(args.seed, kDomainRowChain, args.iteration, r);
            for (uint32_t e = e0; e < e1 && remaining > 0; ++e) {
                const double prob = val[e] * a[col[e]] / s;
                if (prob > 0.0) {
                    const uint32_t drawn = sampleBinomial(rng, remaining, fmin(1.0, prob / remaining_prob));
                    if (drawn) atomicAdd(&counts[col[e]], static_cast<unsigned long long>(drawn));
                    remaining -= drawn;
                }
                remaining_prob -= prob;
            }
            to_noise += remaining;
        }
    } else {
        // a wavefront per row
        const uint32_t lane = threadIdx.x & 63;
        for (uint32_t r = r0 + (threadIdx.x >> 6); r < r1; r += kGibbsBlock / 64) {
            const uint32_t e0 = __builtin_amdgcn_readfirstlane(off[r]), e1 = __builtin_amdgcn_readfirstlane(off[r + 1]);
            const uint32_t reads = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(cnt[r]));
            if (reads == 0) continue;
            double x = 0.0;
            for (uint32_t e = e0 + lane; e < e1; e += 64) x += val[e] * a[col[e]];
            const double s = waveSumF64(x) + nzv[r] * a_noise;
            if (reads <= kCategoricalMaxReads) {
                // Read k falls where u_k s lands among the prefix sums of the row's terms (entries in order, noise behind
                // them); u_k is the k-th uniform of the row's stream, whichever lane draws it.
                double t = 0.0;
                if (lane < reads) {
                    Philox rng = gibbsGenerator(args.seed, kDomainRowCategorical, args.iteration, r);
                    rng.ctr[0] = lane >> 1;
                    double u = rng.uniform();
                    if (lane & 1) u = rng.uniform();
                    t = u * s;
                }
                unsigned long long pending = reads == 64 ? ~0ull : ((1ull << reads) - 1);  // the reads without a column so far
                double base = 0.0;
                for (uint32_t c0 = e0; c0 < e1 && pending; c0 += 64) {
                    const uint32_t e = c0 + lane;
                    const bool ok = e < e1;
                    const uint32_t cj = ok ? col[e] : 0u;
                    double incl = ok ? val[e] * a[cj] : 0.0;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const double up = __shfl_up(incl, d, 64);
                        if (lane >= static_cast<uint32_t>(d)) incl += up;
                    }
                    incl += base;
                    uint32_t mine = 0;
                    for (unsigned long long todo = pending; todo; todo &= todo - 1) {
                        const int k = __builtin_ctzll(todo);
                        const double tk = readLaneF64(t, k);
                        const unsigned long long hit = __ballot(ok && tk < incl);
                        if (hit) {
                            if (lane == static_cast<uint32_t>(__builtin_ctzll(hit))) ++mine;
                            pending &= ~(1ull << k);
                        }
                    }
                    // (the columns of one row are distinct)
                    if (mine) atomicAdd(&counts[cj], static_cast<unsigned long long>(mine));
                    base = readLaneF64(incl, 63);
                }
                if (lane == 0) to_noise += static_cast<unsigned long long>(__builtin_popcountll(pending));
            } else {
                // the chain of binomials over the terms the wave computed: every lane runs the same chain (one generator
                // state, one stream of draws), the lane that holds an entry keeps its draw
                uint32_t remaining = reads;
                double remaining_prob = 1.0;
                Philox rng = gibbsGenerator(args.seed, kDomainRowChain, args.iteration, r);
                for (uint32_t c0 = e0; c0 < e1 && remaining > 0; c0 += 64) {
                    const uint32_t e = c0 + lane;
                    const bool ok = e < e1;
                    const uint32_t cj = ok ? col[e] : 0u;
                    const double prob_mine = ok ? val[e] * a[cj] / s : 0.0;
                    const uint32_t held = min(64u, e1 - c0);
                    uint32_t mine = 0;
                    for (uint32_t j = 0; j < held && remaining > 0; ++j) {
                        const double prob = readLaneF64(prob_mine, static_cast<int>(j));
                        if (prob > 0.0) {
                            const uint32_t drawn = sampleBinomial(rng, remaining, fmin(1.0, prob / remaining_prob));
                            if (lane == j) mine = drawn;
                            remaining -= drawn;
                        }
                        remaining_prob -= prob;
                    }
                    if (mine) atomicAdd(&counts[cj], static_cast<unsigned long long>(mine));
                }
                if (lane == 0) to_noise += remaining;
            }
        }
    }
    if (to_noise) atomicAdd(noise_word, to_noise);
    __syncthreads();
    if (LDS_COLS) {
        for (uint32_t j = threadIdx.x; j < C; j += kGibbsBlock) {
            const unsigned long long cj = c_lds[j];
            if (cj) atomicAdd(&args.counts[j], cj);
        }
    } else if (threadIdx.x == 0 && c_lds[0]) {
        atomicAdd(&args.counts[noise_col], c_lds[0]);
    }
}

struct GibbsUpdateArgs {
    uint32_t problem, C, iteration;
    uint64_t seed;
    double gamma;
    const double * zero_mass;        // [P]
    unsigned long long * counts;     // [C]
    double * g;                      // [C]
    double * partials;               // [ceil(C / kGibbsBlock)]
};

// A workgroup per kGibbsBlock columns, whatever the GPU: the partial sums — and so the total — are a function of C alone.
__global__ __launch_bounds__(kGibbsBlock) void gibbsGridUpdateKernel(const GibbsUpdateArgs args) {
    __shared__ double red[kGibbsBlock / 64];
    const uint32_t j = blockIdx.x * kGibbsBlock + threadIdx.x;
    double g = 0.0;
    if (j < args.C) {
        Philox rng = gibbsGenerator(args.seed, kDomainColumn, args.iteration, j);
        g = sampleGamma(rng, static_cast<double>(args.counts[j]) + args.gamma);
        args.g[j] = g;
        args.counts[j] = (j + 1 == args.C) ? static_cast<unsigned long long>(args.zero_mass[args.problem]) : 0ull;
    }
    const double sum = gibbsBlockSum(g, red);
    if (threadIdx.x == 0) args.partials[blockIdx.x] = sum;
}

struct GibbsRecordArgs {
    uint32_t problem, C, num_partials, recorded;
    const double * total_mass;       // [P]
    const double * g;
    const double * partials;
    double * abundance_out;          // [num_samples x (C - 1)] of the problem
    double * low_partials;           // [num_samples x num_partials]
    double * noise_base;             // [num_samples]
};

__global__ __launch_bounds__(kGibbsBlock) void gibbsGridRecordKernel(const GibbsRecordArgs args) {
    __shared__ double red[kGibbsBlock / 64];
    const double total = gridTotal(args.partials, args.num_partials, red);
    const double T = args.total_mass[args.problem];
    const uint32_t noise_col = args.C - 1;
    const uint32_t j = blockIdx.x * kGibbsBlock + threadIdx.x;
    double low = 0.0;
    if (j < args.C) {
        const double aj = args.g[j] / total;
        if (j == noise_col) {
            args.noise_base[args.recorded] = aj * T;
        } else if (aj < kMinGibbsAbundance) {
            low = aj * T;
            args.abundance_out[static_cast<uint64_t>(args.recorded) * noise_col + j] = 0.0;
        } else {
            args.abundance_out[static_cast<uint64_t>(args.recorded) * noise_col + j] = aj * T;
        }
    }
    low = gibbsBlockSum(low, red);
    if (threadIdx.x == 0) args.low_partials[static_cast<uint64_t>(args.recorded) * args.num_partials + blockIdx.x] = low;
}

__global__ __launch_bounds__(kGibbsBlock) void gibbsGridNoiseKernel(const uint32_t num_samples, const uint32_t num_partials, const double * __restrict__ low_partials,
                                                                  const double * __restrict__ noise_base, double * __restrict__ noise_out) {
    const uint32_t s = blockIdx.x * kGibbsBlock + threadIdx.x;
    if (s >= num_samples) return;
    const double * part = low_partials + static_cast<uint64_t>(s) * num_partials;
    double low = part[0];
    for (uint32_t b = 1; b < num_partials; ++b) low += part[b];
    noise_out[s] = low + noise_base[s];
}

// the chain starts from the EM estimate (:128-136): g = a, total = 1
__global__ __launch_bounds__(kGibbsBlock) void gibbsGridInitKernel(const uint32_t problem, const uint32_t C, const uint32_t num_partials, const double * __restrict__ init_abundances,
                                                                 const double * __restrict__ init_noise_count, const double * __restrict__ total_mass,
                                                                 const double * __restrict__ zero_mass, double * __restrict__ g,
                                                                 unsigned long long * __restrict__ counts, double * __restrict__ partials) {
    const uint32_t j = blockIdx.x * kGibbsBlock + threadIdx.x;
    if (j < num_partials) partials[j] = (j == 0) ? 1.0 : 0.0;
    if (j >= C) return;
    const bool noise = j + 1 == C;
    g[j] = (noise ? init_noise_count[problem] : init_abundances[j]) / total_mass[problem];
    counts[j] = noise ? static_cast<unsigned long long>(zero_mass[problem]) : 0ull;
}

template <int LANES>
void launchSplit(const bool lds_cols, const GibbsSplitArgs & args, const uint32_t grid, hipStream_t st) {
    if (lds_cols) {
        gibbsGridSplitKernel<LANES, true><<<dim3(grid), dim3(kGibbsBlock), 16 * static_cast<size_t>(args.C), st>>>(args);
    } else {
        gibbsGridSplitKernel<LANES, false><<<dim3(grid), dim3(kGibbsBlock), 16, st>>>(args);
    }
}

// lanes per row by the mean row length (em_plan.hpp, emGridRowLanes: a thread per row below six entries; the sampler has the
// two ends of that scale)
inline int gibbsRowLanes(const uint32_t rows, const uint32_t entries) {
    return static_cast<double>(entries) < 12.0 * std::max(1u, rows) ? 1 : 64;
}

}  // namespace

namespace rpvg_hip_detail {

int runGibbsGridProblems(rpvg_hip_ctx * ctx, hipStream_t st, const GibbsGridProblem * problems, const uint32_t count, const GibbsGridStorage & storage,
                         const uint32_t gibbs_thin_its, const double gamma) {
    const uint32_t cus = static_cast<uint32_t>(ctx->props.multiProcessorCount);
    for (uint32_t i = 0; i < count; ++i) {
        const GibbsGridProblem & d = problems[i];
        const uint32_t C = d.columns, rows = d.rows;
        const uint64_t num_its = static_cast<uint64_t>(d.num_samples) * gibbs_thin_its;
        RPVG_REQUIRE(num_its <= 0xffffffffull, "rpvg_hip_gibbs_read_counts: problem %u asks for %llu Gibbs iterations (limit 2^32 - 1)", d.problem,
                     static_cast<unsigned long long>(num_its));
        const int row_lanes = gibbsRowLanes(rows, d.entries);
        const bool lds_cols = 16 * static_cast<size_t>(C) <= kGibbsGridLdsLimit;
        // workgroups: a row slot per row at the most, a few workgroups per CU at the most, and — with the columns in LDS — few
        // enough that their loads and flushes of the column vectors (16 B per column and workgroup) stay below the pass itself
        const uint64_t slots = static_cast<uint64_t>(kGibbsBlock / row_lanes);
        uint64_t blocks = (static_cast<uint64_t>(rows) + slots - 1) / slots;
        blocks = std::min<uint64_t>(blocks, static_cast<uint64_t>(cus) * 4);
        if (lds_cols) blocks = std::min<uint64_t>(blocks, std::max<uint64_t>(16, (static_cast<uint64_t>(rows) + d.entries) / C));
        blocks = std::max<uint64_t>(1, blocks);
        const uint32_t rows_per_block = std::max<uint32_t>(1, static_cast<uint32_t>((static_cast<uint64_t>(rows) + blocks - 1) / blocks));
        const uint32_t grid = std::max<uint32_t>(1, (rows + rows_per_block - 1) / rows_per_block);
        const uint32_t num_partials = (C + kGibbsBlock - 1) / kGibbsBlock;

        DeviceBuffer<double> d_g, d_partials, d_low_partials, d_noise_base;
        DeviceBuffer<unsigned long long> d_counts;
        RPVG_HIP_CHECK(d_g.alloc(C));
        RPVG_HIP_CHECK(d_counts.alloc(C));
        RPVG_HIP_CHECK(d_partials.alloc(num_partials));
        RPVG_HIP_CHECK(d_low_partials.alloc(static_cast<size_t>(d.num_samples) * num_partials));
        RPVG_HIP_CHECK(d_noise_base.alloc(d.num_samples));

        GibbsSplitArgs sa;
        sa.problem = d.problem;
        sa.C = C;
        sa.rows = rows;
        sa.rows_per_block = rows_per_block;
        sa.iteration = 0;
        sa.seed = d.seed;
        sa.row_base = storage.problems.row_base;
        sa.ent_base = storage.problems.ent_base;
        sa.prow_off = storage.problems.prow_off;
        sa.prow_count = storage.problems.prow_count;
        sa.prow_noise = storage.problems.prow_noise;
        sa.pent_col = storage.problems.pent_col;
        sa.pent_val = storage.problems.pent_val;
        sa.g = d_g.ptr;
        sa.counts = d_counts.ptr;
        GibbsUpdateArgs ua;
        ua.problem = d.problem;
        ua.C = C;
        ua.iteration = 0;
        ua.seed = d.seed;
        ua.gamma = gamma;
        ua.zero_mass = storage.problems.zero_mass;
        ua.counts = d_counts.ptr;
        ua.g = d_g.ptr;
        ua.partials = d_partials.ptr;
        GibbsRecordArgs ra;
        ra.problem = d.problem;
        ra.C = C;
        ra.num_partials = num_partials;
        ra.recorded = 0;
        ra.total_mass = storage.problems.total_mass;
        ra.g = d_g.ptr;
        ra.partials = d_partials.ptr;
        ra.abundance_out = storage.abundance_samples + d.abund_sample_off;
        ra.low_partials = d_low_partials.ptr;
        ra.noise_base = d_noise_base.ptr;

        const int span = ctx->spanBegin(FAM_EM_SPARSE, st);
        gibbsGridInitKernel<<<dim3(num_partials), dim3(kGibbsBlock), 0, st>>>(d.problem, C, num_partials, storage.init_abundances + d.col_begin, storage.init_noise_count,
                                                                             storage.problems.total_mass, storage.problems.zero_mass, d_g.ptr, d_counts.ptr, d_partials.ptr);
        for (uint32_t it = 1; it <= num_its; ++it) {
            sa.iteration = ua.iteration = it;
            if (row_lanes == 1) {
                launchSplit<1>(lds_cols, sa, grid, st);
            } else {
                launchSplit<64>(lds_cols, sa, grid, st);
            }
            gibbsGridUpdateKernel<<<dim3(num_partials), dim3(kGibbsBlock), 0, st>>>(ua);
            if (it % gibbs_thin_its == 0) {
                gibbsGridRecordKernel<<<dim3(num_partials), dim3(kGibbsBlock), 0, st>>>(ra);
                ++ra.recorded;
            }
        }
        gibbsGridNoiseKernel<<<dim3((d.num_samples + kGibbsBlock - 1) / kGibbsBlock), dim3(kGibbsBlock), 0, st>>>(d.num_samples, num_partials, d_low_partials.ptr,
                                                                                                                    d_noise_base.ptr, storage.noise_samples + d.sample_off);
        const hipError_t launched = hipGetLastError();
        ctx->spanEnd(span);  // (closed on the error path too)
        RPVG_HIP_CHECK(launched);
        RPVG_HIP_CHECK(waitStream(st));  // (the buffers of this problem go back to the pool)
        ctx->stats.gibbs_count_grid_problems += 1;
        ctx->stats.gibbs_count_grid_iterations += num_its;
    }
    return RPVG_HIP_OK;
}

}  // namespace rpvg_hip_detail

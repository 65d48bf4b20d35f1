// The read-count Gibbs sampler (-n) on the compacted problems of an EM solve (gfx950).
//
// gibbsReadCountSampler (src/path_abundance_estimator.cpp:116-212) for a batch of problems: per Gibbs
// iteration every row's reads are split multinomially over its columns with probabilities
// P_ij a_j / s_i (the reference draws the multinomial as a chain of binomials, :149-178), then every
// component draws a_j ~ Gamma(count_j + gamma, 1) and the vector is renormalised (:182-190); every
// `thin`-th state is recorded (:192-210).  ONE workgroup per problem runs all iterations (a problem too
// wide for its LDS or too large for one workgroup takes the whole GPU instead: gibbs_grid.hip).  The
// reference's mt19937 / libstdc++ distribution streams cannot be reproduced on a GPU:
// draws come from the counter-based Philox4x32-10 generator keyed by the problem's seed (gibbs_random.hpp),
// so parity with the reference is statistical.  Rows without any selected path put all their reads on the
// noise component (their posterior there is exactly 1), as in the EM kernel.

#include "em_block.hpp"
#include "gibbs_random.hpp"
#include "gibbs_samples.hpp"

#include <vector>

using namespace rpvg_hip_detail;

namespace {

struct GibbsLaunchArgs {
    uint32_t count;
    EmProblemsView problems;
    const double * init_abundances;   // [col_off[P]] expected counts (EM result)
    const double * init_noise_count;  // [P]
    const uint32_t * num_samples;     // [P]
    const uint64_t * seed;            // [P]
    const uint64_t * sample_off;      // [P+1]
    const uint64_t * abund_sample_off;  // [P+1] prefix of num_samples * columns
    uint32_t thin;
    double gamma;
    double * noise_samples;
    double * abundance_samples;
};

constexpr double kMinGibbsAbundance = 1e-8;  // src/path_abundance_estimator.cpp:14

__global__ __launch_bounds__(256) void gibbsReadCountKernel(const GibbsLaunchArgs args) {
    constexpr int BLOCK = 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t p = blockIdx.x;
    if (p >= args.count) return;
    const uint32_t n_samples = args.num_samples[p];
    if (n_samples == 0) return;
    const uint32_t C = args.problems.paths(p) + 1;
    const uint32_t noise_col = C - 1;
    double * a = reinterpret_cast<double *>(smem_raw);          // [C]
    double * red = a + C;                                       // [BLOCK/64 + 2]
    unsigned long long * counts = reinterpret_cast<unsigned long long *>(red + (BLOCK / 64 + 2));  // [C]

    const EmProblemRows csr = args.problems.rows(p);
    const uint32_t n_rows = csr.rows;
    const uint32_t * off = csr.off;
    const double * cnt = csr.count;
    const double * nzv = csr.noise;
    const uint32_t * col = csr.col;
    const double * val = csr.val;
    const double T = args.problems.total_mass[p];
    const unsigned long long Z = static_cast<unsigned long long>(args.problems.zero_mass[p]);

    // start from the EM estimate (:128-136)
    for (uint32_t j = threadIdx.x; j < C; j += BLOCK) {
        a[j] = (j == noise_col ? args.init_noise_count[p] : args.init_abundances[args.problems.col_off[p] + j]) / T;
    }
    __syncthreads();

    Philox rng;
    rng.init(args.seed[p], p, threadIdx.x);

    double * noise_out = args.noise_samples + args.sample_off[p];
    double * abund_out = args.abundance_samples + args.abund_sample_off[p];
    const uint32_t num_its = n_samples * args.thin;
    uint32_t recorded = 0;

    for (uint32_t it = 1; it <= num_its; ++it) {
        for (uint32_t j = threadIdx.x; j < C; j += BLOCK) counts[j] = (j == noise_col) ? Z : 0ull;
        __syncthreads();
        const double a_noise = a[noise_col];
        for (uint32_t r = threadIdx.x; r < n_rows; r += BLOCK) {
            const uint32_t e0 = off[r], e1 = off[r + 1];
            const double nz = nzv[r];
            double s = nz * a_noise;
            for (uint32_t e = e0; e < e1; ++e) s += val[e] * a[col[e]];
            uint32_t remaining = static_cast<uint32_t>(cnt[r]);
            double remaining_prob = 1.0;
            for (uint32_t e = e0; e < e1 && remaining > 0; ++e) {
                const double prob = val[e] * a[col[e]] / s;
                if (prob > 0.0) {
                    const uint32_t drawn = sampleBinomial(rng, remaining, fmin(1.0, prob / remaining_prob));
                    if (drawn) atomicAdd(&counts[col[e]], static_cast<unsigned long long>(drawn));
                    remaining -= drawn;
                }
                remaining_prob -= prob;
            }
            if (remaining) atomicAdd(&counts[noise_col], static_cast<unsigned long long>(remaining));
        }
        __syncthreads();
        double local = 0.0;
        for (uint32_t j = threadIdx.x; j < C; j += BLOCK) {
            const double g = sampleGamma(rng, static_cast<double>(counts[j]) + args.gamma);
            a[j] = g;
            local += g;
        }
        const double total = blockReduceSum<double, BLOCK>(local, red);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < C; j += BLOCK) a[j] = a[j] / total;
        __syncthreads();
        if (it % args.thin == 0) {
            double low = 0.0;
            for (uint32_t j = threadIdx.x; j < noise_col; j += BLOCK) {
                const double aj = a[j];
                if (aj < kMinGibbsAbundance) {
                    low += aj * T;
                    abund_out[static_cast<uint64_t>(recorded) * noise_col + j] = 0.0;
                } else {
                    abund_out[static_cast<uint64_t>(recorded) * noise_col + j] = aj * T;
                }
            }
            low = blockReduceSum<double, BLOCK>(low, red);
            if (threadIdx.x == 0) noise_out[recorded] = low + a[noise_col] * T;
            ++recorded;
            __syncthreads();
        }
    }
}
}  // namespace

namespace {

// what a call needs on the device besides its samples; it goes back to the pool once the stream has been waited for
struct GibbsCallBuffers {
    DeviceBuffer<uint32_t> d_kept_rows, d_kept_ent, d_num_samples;
    DeviceBuffer<double> d_total, d_init_abund, d_init_noise;
    DeviceBuffer<uint64_t> d_seed;
    HostProblemSet ps;
};

// Everything of rpvg_hip_gibbs_read_counts up to its two downloads: validates, draws every sample and leaves them in `s` with
// their offsets (queued on the context's stream, not waited for).  The caller holds the context's lock, waits for the stream and
// lets `call` go only then.  *drawn: whether anything was queued (a call with no problem or no sample leaves `s` empty).
int drawGibbsSamples(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_em_problems * problems, const double * init_abundances,
                     const double * init_noise_count, const uint32_t * num_samples, const uint64_t * seeds, const uint32_t gibbs_thin_its,
                     const double gamma, const char * who, GibbsCallBuffers & call, rpvg_hip_gibbs_samples & s, bool * drawn) {
    *drawn = false;
    const uint32_t P = problems->num_problems;
    s.num_problems = P;
    s.sample_off.assign(static_cast<size_t>(P) + 1, 0);
    s.abund_sample_off.assign(static_cast<size_t>(P) + 1, 0);
    if (P == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(problems->cluster && problems->col_off && problems->col_path, "%s: NULL problem arrays", who);
    RPVG_REQUIRE(init_abundances && init_noise_count && num_samples && seeds, "%s: NULL argument", who);
    RPVG_REQUIRE(gibbs_thin_its > 0, "%s: gibbs_thin_its must be positive", who);
    RPVG_REQUIRE(gamma >= 1.0, "%s: gamma must be >= 1 (the reference uses 1)", who);

    std::vector<uint64_t> & sample_off = s.sample_off, & abund_sample_off = s.abund_sample_off;
    for (uint32_t p = 0; p < P; ++p) {
        sample_off[p + 1] = sample_off[p] + num_samples[p];
        abund_sample_off[p + 1] = abund_sample_off[p] + static_cast<uint64_t>(num_samples[p]) * (problems->col_off[p + 1] - problems->col_off[p]);
    }
    if (sample_off[P] == 0) return RPVG_HIP_OK;

    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // the compacted CSR of the problems, as for the EM (the first stage of a solve: no EM kernels)
    DeviceBuffer<uint32_t> & d_kept_rows = call.d_kept_rows, & d_kept_ent = call.d_kept_ent;
    DeviceBuffer<double> & d_total = call.d_total;
    RPVG_HIP_CHECK(d_kept_rows.alloc(P));
    RPVG_HIP_CHECK(d_kept_ent.alloc(P));
    RPVG_HIP_CHECK(d_total.alloc(P));
    EmOutputs out{nullptr, nullptr, nullptr, d_kept_rows.ptr, d_kept_ent.ptr, d_total.ptr};
    HostProblemSet & ps = call.ps;
    int rc = prepareHostProblems(ctx, batch, problems, ps, out, who);
    if (rc != RPVG_HIP_OK) return rc;
    {
        const EmSolveKnobs knobs = emSolveKnobs();
        int build_span = -1;
        rc = queueEmFill(ctx, batch, ps.list, out, ps.work, knobs, planEmFill(emSolveShape(ctx, ps.list, false), knobs), false, build_span);
        if (rc != RPVG_HIP_OK) return rc;
        ctx->spanEnd(build_span);
    }
    const EmProblemsView view = ps.work.view(ps.list, out);

    // Two routes (em_plan.hpp: gibbsTakesGrid).  A problem whose columns do not fit gibbsReadCountKernel's LDS-resident vectors,
    // or whose kept rows + entries reach gibbsGridMinWork() (0: never for its size — a problem too wide still goes), takes the
    // whole GPU per iteration (gibbs_grid.hip).  The host has to see the counts for that: only a call that sits on a cluster
    // large enough, or has a problem wide enough, pays for the look (the gate of a solve's grid_possible).  Every other
    // problem runs on one workgroup, under its index in the call: the launch covers all problems, the grid ones with no
    // samples to draw.
    const uint64_t grid_min_work = gibbsGridMinWork();
    const bool grid_possible = gibbsGridPossible(ps.list.max_cols, ps.list.max_cluster_work, grid_min_work);
    std::vector<uint32_t> staying_samples;  // num_samples with the grid problems masked out
    std::vector<GibbsGridProblem> grid_problems;
    uint32_t staying_max_cols = ps.list.max_cols;
    bool any_staying = true;
    if (grid_possible) {
        std::vector<uint32_t> kept_rows(P), kept_ent(P);
        RPVG_HIP_CHECK(d_kept_rows.download(kept_rows.data(), st));
        RPVG_HIP_CHECK(d_kept_ent.download(kept_ent.data(), st));
        RPVG_HIP_CHECK(waitStream(st));
        staying_samples.assign(num_samples, num_samples + P);
        staying_max_cols = 1;
        any_staying = false;
        for (uint32_t p = 0; p < P; ++p) {
            if (num_samples[p] == 0) continue;
            const uint32_t C = static_cast<uint32_t>(problems->col_off[p + 1] - problems->col_off[p]) + 1;
            if (!gibbsTakesGrid(C, kept_rows[p], kept_ent[p], grid_min_work)) {
                staying_max_cols = std::max(staying_max_cols, C);
                any_staying = true;
                continue;
            }
            staying_samples[p] = 0;
            GibbsGridProblem g;
            g.problem = p;
            g.columns = C;
            g.rows = kept_rows[p];
            g.entries = kept_ent[p];
            g.num_samples = num_samples[p];
            g.pad = 0;
            g.col_begin = problems->col_off[p];
            g.sample_off = sample_off[p];
            g.abund_sample_off = abund_sample_off[p];
            g.seed = seeds[p];
            grid_problems.push_back(g);
        }
    }

    DeviceBuffer<double> & d_init_abund = call.d_init_abund, & d_init_noise = call.d_init_noise;
    DeviceBuffer<double> & d_noise_samples = s.d_noise_samples, & d_abund_samples = s.d_abund_samples;
    DeviceBuffer<uint32_t> & d_num_samples = call.d_num_samples;
    DeviceBuffer<uint64_t> & d_seed = call.d_seed, & d_sample_off = s.d_sample_off, & d_abund_sample_off = s.d_abund_sample_off;
    RPVG_HIP_CHECK(d_init_abund.upload(init_abundances, ps.n_cols_total, st));
    RPVG_HIP_CHECK(d_init_noise.upload(init_noise_count, P, st));
    RPVG_HIP_CHECK(d_num_samples.upload(grid_problems.empty() ? num_samples : staying_samples.data(), P, st));
    RPVG_HIP_CHECK(d_seed.upload(seeds, P, st));
    RPVG_HIP_CHECK(d_sample_off.upload(sample_off.data(), P + 1, st));
    RPVG_HIP_CHECK(d_abund_sample_off.upload(abund_sample_off.data(), P + 1, st));
    RPVG_HIP_CHECK(d_noise_samples.alloc(sample_off[P]));
    RPVG_HIP_CHECK(d_abund_samples.alloc(abund_sample_off[P]));

    // the grid problems run next to the one-workgroup kernel: on a stream of their own (the EM's first, em_grid.hip), behind what
    // `st` holds so far — the compacted CSR and the uploads
    hipStream_t grid_st = st;
    if (any_staying && !grid_problems.empty()) {
        hipError_t e = hipSuccess;
        if (!ctx->grid_stream[0]) e = hipStreamCreateWithFlags(&ctx->grid_stream[0], hipStreamNonBlocking);
        if (e == hipSuccess && !ctx->grid_ready) e = hipEventCreateWithFlags(&ctx->grid_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ctx->grid_ready, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->grid_stream[0], ctx->grid_ready, 0);
        RPVG_HIP_CHECK(e);
        grid_st = ctx->grid_stream[0];
    }
    if (any_staying) {
        GibbsLaunchArgs args;
        args.count = P;
        args.problems = view;
        args.init_abundances = d_init_abund.ptr;
        args.init_noise_count = d_init_noise.ptr;
        args.num_samples = d_num_samples.ptr;
        args.seed = d_seed.ptr;
        args.sample_off = d_sample_off.ptr;
        args.abund_sample_off = d_abund_sample_off.ptr;
        args.thin = gibbs_thin_its;
        args.gamma = gamma;
        args.noise_samples = d_noise_samples.ptr;
        args.abundance_samples = d_abund_samples.ptr;

        // (sized by the widest problem that stays)
        const size_t lds = gibbsOneWorkgroupLds(staying_max_cols);
        if (lds > kLdsOptIn) {
            RPVG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&gibbsReadCountKernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        }
        const int span = ctx->spanBegin(FAM_EM_SPARSE);
        gibbsReadCountKernel<<<dim3(P), dim3(256), lds, st>>>(args);
        ctx->spanEnd(span);
        RPVG_HIP_CHECK(hipGetLastError());
    }
    if (!grid_problems.empty()) {
        GibbsGridStorage storage;
        storage.problems = view;
        storage.init_abundances = d_init_abund.ptr;
        storage.init_noise_count = d_init_noise.ptr;
        storage.noise_samples = d_noise_samples.ptr;
        storage.abundance_samples = d_abund_samples.ptr;
        // (waits for grid_st behind every problem: their samples are in place when the caller queues its downloads)
        rc = runGibbsGridProblems(ctx, grid_st, grid_problems.data(), static_cast<uint32_t>(grid_problems.size()), storage, gibbs_thin_its, gamma);
        if (rc != RPVG_HIP_OK) {
            (void) hipDeviceSynchronize();  // (the buffers of this call go back to the pool on return)
            return rc;
        }
    }
    *drawn = true;
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" int rpvg_hip_gibbs_read_counts(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch,
                                          const rpvg_hip_em_problems * problems, const double * init_abundances,
                                          const double * init_noise_count, const uint32_t * num_samples,
                                          const uint64_t * seeds, uint32_t gibbs_thin_its, double gamma,
                                          double * noise_samples, double * abundance_samples) {
    RPVG_REQUIRE(ctx && batch && problems, "rpvg_hip_gibbs_read_counts: NULL argument");
    RPVG_REQUIRE(problems->num_problems == 0 || (noise_samples && abundance_samples), "rpvg_hip_gibbs_read_counts: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    GibbsCallBuffers call;
    rpvg_hip_gibbs_samples samples;
    bool drawn = false;
    const int rc = drawGibbsSamples(ctx, batch, problems, init_abundances, init_noise_count, num_samples, seeds, gibbs_thin_its, gamma,
                                    "rpvg_hip_gibbs_read_counts", call, samples, &drawn);
    if (rc != RPVG_HIP_OK || !drawn) return rc;
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(samples.d_noise_samples.download(noise_samples, st));
    RPVG_HIP_CHECK(samples.d_abund_samples.download(abundance_samples, st));
    RPVG_HIP_CHECK(waitStream(st));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_gibbs_read_counts_resident(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_em_problems * problems,
                                                   const double * init_abundances, const double * init_noise_count,
                                                   const uint32_t * num_samples, const uint64_t * seeds, uint32_t gibbs_thin_its,
                                                   double gamma, rpvg_hip_gibbs_samples ** samples_out) {
    RPVG_REQUIRE(ctx && batch && problems && samples_out, "rpvg_hip_gibbs_read_counts_resident: NULL argument");
    *samples_out = nullptr;
    std::unique_ptr<rpvg_hip_gibbs_samples> samples(new (std::nothrow) rpvg_hip_gibbs_samples());
    if (!samples) {
        setError("rpvg_hip_gibbs_read_counts_resident: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    std::lock_guard<std::mutex> lock(ctx->mutex);
    GibbsCallBuffers call;
    bool drawn = false;
    const int rc = drawGibbsSamples(ctx, batch, problems, init_abundances, init_noise_count, num_samples, seeds, gibbs_thin_its, gamma,
                                    "rpvg_hip_gibbs_read_counts_resident", call, *samples, &drawn);
    if (rc != RPVG_HIP_OK) return rc;
    if (drawn) RPVG_HIP_CHECK(waitStream(ctx->stream));  // (the buffers of the call go back to the pool on return)
    *samples_out = samples.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_gibbs_samples_get(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_samples * samples, double * noise_samples,
                                          double * abundance_samples) {
    RPVG_REQUIRE(ctx && samples, "rpvg_hip_gibbs_samples_get: NULL argument");
    RPVG_REQUIRE((samples->d_noise_samples.count == 0 || noise_samples) && (samples->d_abund_samples.count == 0 || abundance_samples),
                 "rpvg_hip_gibbs_samples_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(samples->d_noise_samples.download(noise_samples, st));
    RPVG_HIP_CHECK(samples->d_abund_samples.download(abundance_samples, st));
    RPVG_HIP_CHECK(waitStream(st));
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_gibbs_samples_free(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_samples * samples) {
    if (!samples) return;
    if (ctx) {  // nothing queued on the context's stream may still use the buffers
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
    }
    delete samples;
}

// frag_length.hip — the fragment-length model of a paired-end run on the GPU (interface include/rpvg_frag.h, rpvg_hip.h).
//
// Takes over   FragmentLengthDist(frag_length_counts, skew_normal)      src/fragment_length_dist.cpp:60-285
//              FragmentLengthDist::logProb as a table                   src/fragment_length_dist.cpp:385-427
//              PathsIndex::effectivePathLength                          src/paths_index.cpp:190-229
//              Utils::truncated_skew_normal_expected_value              src/utils.hpp:229-247
//
// fragLengthFitKernel       The whole fit in ONE launch of ONE workgroup of 1024 threads.  The fit is some hundreds to
//                           thousands of log-likelihood sums that depend on each other (golden-section searches inside
//                           bracketing loops inside an alternating outer loop): a launch per sum would cost more than
//                           the sum.  Thread t keeps counts t, t + 1024, ... in registers (at most 64; the kernel is
//                           compiled for 1, 4, 16 and 64 entries per thread).  One sum = the thread's entries in
//                           ascending index, a shuffle tree over the wavefront, the 16 wavefront partials through LDS
//                           added in wavefront order by every thread: one fixed order, so two runs give the same bits,
//                           and every thread holds the same value and walks the same scalar control flow
//                           (frag_math.hpp, fitFragmentLengths).  One barrier per sum (two LDS rows, used alternately).
//                           Latency-bound by construction: a single resident workgroup, most lanes idle behind the
//                           zero counts, FP64 erfc / log on the critical path.
// fragLengthTableKernel     logProb(v) for v = 0 .. 65535 into the table read_rows.hip reads.
// effectiveLengthKernel     one lane per path; the terms of the lower bound c = 1 come from effectiveLengthLowerKernel
//                           (one thread, once per launch).
// fragLengthEvalKernel      skew-normal CDF, truncated mean and Owen's T for rows of arguments (tests, measurements).

#include <memory>

#include "../../include/rpvg_rows.h"
#include "common.hpp"
#include "frag_length.hpp"
#include "frag_math.hpp"

using namespace rpvg_hip_detail;

namespace {

constexpr int kFitThreads = 1024;
constexpr int kFitWaves = kFitThreads / 64;

static_assert(sizeof(rpvg_frag::FitResult) == sizeof(rpvg_frag_length_fit), "FitResult is rpvg_frag_length_fit");
static_assert(sizeof(rpvg_frag::EffectiveLengthLower) == 5 * sizeof(double), "EffectiveLengthLower is five doubles");

const rpvg_frag::GaussLegendre & gaussLegendre() {
    static const rpvg_frag::GaussLegendre gl = rpvg_frag::makeGaussLegendre();
    return gl;
}

// The sums of the fit over the counts of one workgroup; every thread gets the same total.
template <int E>
struct BlockSums {
    uint32_t c[E];     // counts tid, tid + 1024, ... (0 beyond the vector)
    uint32_t tid;
    uint32_t parity;
    double * partials;  // LDS [2][kFitWaves]

    __device__ double reduce(double v) {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        // Two rows used alternately: a wavefront that writes row p again has passed the barrier of the sum in between,
        // which every wavefront reaches only after it has read row p.
        double * row = partials + (parity & 1u) * kFitWaves;
        ++parity;
        if ((tid & 63u) == 0) row[tid >> 6] = v;
        __syncthreads();
        double total = 0;
        for (int w = 0; w < kFitWaves; ++w) total += row[w];
        return total;
    }

    __device__ void moments(double * k0, double * k1, double * k2, double * k3) {
        uint64_t size = 0, sum = 0;
        double s2 = 0, s3 = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint64_t i = tid + static_cast<uint64_t>(j) * kFitThreads;
            size += c[j];
            sum += i * c[j];
            double term = static_cast<double>(c[j] * i * i);
            s2 += term;
            term *= i;
            s3 += term;
        }
        // below 2^53: the double sums of these integers are exact in any order
        *k0 = reduce(static_cast<double>(size));
        *k1 = reduce(static_cast<double>(sum));
        *k2 = reduce(s2);
        *k3 = reduce(s3);
    }

    __device__ double squaredDeviations(const double mu) {
        double total = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint64_t i = tid + static_cast<uint64_t>(j) * kFitThreads;
            const double dev = i - mu;
            total += c[j] * dev * dev;
        }
        return reduce(total);
    }

    __device__ double variance(const double loc) {
        double total = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint64_t i = tid + static_cast<uint64_t>(j) * kFitThreads;
            total += pow(static_cast<double>(i) - loc, 2) * c[j];
        }
        return reduce(total);
    }

    __device__ double logLikelihood(const double mu, const double sigma, const double alpha) {
        double ll = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (c[j] == 0) continue;
            const uint64_t i = tid + static_cast<uint64_t>(j) * kFitThreads;
            ll += c[j] * rpvg_frag::logSkewNormalPdf(static_cast<double>(i), mu, sigma, alpha);
        }
        return reduce(ll);
    }
};

template <int E>
__global__ __launch_bounds__(kFitThreads) void fragLengthFitKernel(const uint32_t * __restrict__ counts, const uint32_t n, const int skew_normal,
                                                                   rpvg_frag::FitResult * __restrict__ out) {
    __shared__ double partials[2 * kFitWaves];
    BlockSums<E> sums;
    sums.tid = threadIdx.x;
    sums.parity = 0;
    sums.partials = partials;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const uint32_t i = threadIdx.x + static_cast<uint32_t>(j) * kFitThreads;
        sums.c[j] = (i < n) ? counts[i] : 0u;
    }
    const rpvg_frag::FitResult fit = rpvg_frag::fitFragmentLengths(sums, n, skew_normal != 0);
    if (threadIdx.x == 0) *out = fit;
}

__global__ __launch_bounds__(256) void fragLengthTableKernel(const double loc, const double scale, const double shape, double * __restrict__ table) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < RPVG_FRAG_LENGTH_TABLE_SIZE) table[v] = rpvg_frag::logProb(static_cast<double>(v), loc, scale, shape);
}

__global__ void effectiveLengthLowerKernel(const double loc, const double scale, const double shape, const rpvg_frag::GaussLegendre gl,
                                           rpvg_frag::EffectiveLengthLower * __restrict__ lower) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *lower = rpvg_frag::effectiveLengthLower(loc, scale, shape, gl);
}

__global__ __launch_bounds__(256) void effectiveLengthKernel(const uint64_t n, const uint32_t * __restrict__ path_length, const double loc,
                                                             const double scale, const double shape, const rpvg_frag::GaussLegendre gl,
                                                             const rpvg_frag::EffectiveLengthLower * __restrict__ lower_in,
                                                             double * __restrict__ out) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const rpvg_frag::EffectiveLengthLower lower = *lower_in;
    out[p] = rpvg_frag::effectivePathLength(path_length[p], loc, scale, shape, lower, gl);
}

__global__ __launch_bounds__(256) void fragLengthEvalKernel(const uint64_t n, const int what, const double * __restrict__ rows,
                                                            const rpvg_frag::GaussLegendre gl, double * __restrict__ out) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double * a = rows + r * 5;
    double value;
    if (what == 0) {
        value = rpvg_frag::skewNormalCdf(a[0], a[1], a[2], a[3], gl);
    } else if (what == 1) {
        value = rpvg_frag::truncatedSkewNormalMean(a[0], a[1], a[2], a[3], a[4], gl);
    } else {
        value = rpvg_frag::owensT(a[0], a[1], gl);
    }
    out[r] = value;
}

inline dim3 gridOf(const uint64_t n, const uint32_t block) { return dim3(static_cast<uint32_t>((n + block - 1) / block)); }

}  // namespace

int rpvg_hip_detail::launchEffectiveLengths(hipStream_t st, const double loc, const double scale, const double shape, const uint32_t * d_length,
                                            const uint64_t n, double * d_out, DeviceBuffer<double> & lower_scratch) {
    if (n == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(n < (1ull << 39), "effective lengths: %llu paths exceed one launch", static_cast<unsigned long long>(n));
    RPVG_HIP_CHECK(lower_scratch.alloc(sizeof(rpvg_frag::EffectiveLengthLower) / sizeof(double)));
    rpvg_frag::EffectiveLengthLower * lower = reinterpret_cast<rpvg_frag::EffectiveLengthLower *>(lower_scratch.ptr);
    effectiveLengthLowerKernel<<<dim3(1), dim3(64), 0, st>>>(loc, scale, shape, gaussLegendre(), lower);
    effectiveLengthKernel<<<gridOf(n, 256), dim3(256), 0, st>>>(n, d_length, loc, scale, shape, gaussLegendre(), lower, d_out);
    RPVG_HIP_CHECK(hipGetLastError());
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_frag_length_fit(rpvg_hip_ctx * ctx, const uint32_t * counts, uint32_t n, int skew_normal, rpvg_frag_length_fit * out) {
    RPVG_REQUIRE(ctx && counts && out, "rpvg_hip_frag_length_fit: NULL argument");
    RPVG_REQUIRE(n > 0, "rpvg_hip_frag_length_fit: no counts");
    RPVG_REQUIRE(n <= RPVG_FRAG_LENGTH_MAX_COUNTS, "rpvg_hip_frag_length_fit: %u counts, a fragment length has 16 bits", n);
    RPVG_REQUIRE(counts[0] == 0, "rpvg_hip_frag_length_fit: fragments of length 0 counted");

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<uint32_t> d_counts;
    DeviceBuffer<rpvg_frag::FitResult> d_fit;
    RPVG_HIP_CHECK(d_counts.upload(counts, n, st));
    RPVG_HIP_CHECK(d_fit.alloc(1));
    rpvg_frag::FitResult * fit = d_fit.ptr;
    if (n <= 1 * kFitThreads) {
        fragLengthFitKernel<1><<<dim3(1), dim3(kFitThreads), 0, st>>>(d_counts.ptr, n, skew_normal, fit);
    } else if (n <= 4 * kFitThreads) {
        fragLengthFitKernel<4><<<dim3(1), dim3(kFitThreads), 0, st>>>(d_counts.ptr, n, skew_normal, fit);
    } else if (n <= 16 * kFitThreads) {
        fragLengthFitKernel<16><<<dim3(1), dim3(kFitThreads), 0, st>>>(d_counts.ptr, n, skew_normal, fit);
    } else {
        fragLengthFitKernel<64><<<dim3(1), dim3(kFitThreads), 0, st>>>(d_counts.ptr, n, skew_normal, fit);
    }
    RPVG_HIP_CHECK(hipGetLastError());
    rpvg_frag::FitResult h_fit;
    RPVG_HIP_CHECK(d_fit.download(&h_fit, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    std::memcpy(out, &h_fit, sizeof(h_fit));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_frag_length_table(rpvg_hip_ctx * ctx, double loc, double scale, double shape, rpvg_hip_frag_table ** out) {
    RPVG_REQUIRE(ctx && out, "rpvg_hip_frag_length_table: NULL argument");
    *out = nullptr;
    RPVG_REQUIRE(loc >= 0 && scale > 0 && std::isfinite(loc) && std::isfinite(scale) && std::isfinite(shape),
                 "rpvg_hip_frag_length_table: not a valid distribution (loc %g, scale %g, shape %g)", loc, scale, shape);
    std::unique_ptr<rpvg_hip_frag_table> table(new (std::nothrow) rpvg_hip_frag_table());
    if (!table) {
        setError("rpvg_hip_frag_length_table: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    table->loc = loc;
    table->scale = scale;
    table->shape = shape;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(table->log_prob.alloc(RPVG_FRAG_LENGTH_TABLE_SIZE));
    fragLengthTableKernel<<<gridOf(RPVG_FRAG_LENGTH_TABLE_SIZE, 256), dim3(256), 0, st>>>(loc, scale, shape, table->log_prob.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    *out = table.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_frag_length_table_get(rpvg_hip_ctx * ctx, const rpvg_hip_frag_table * table, double * log_prob_out) {
    RPVG_REQUIRE(ctx && table && log_prob_out, "rpvg_hip_frag_length_table_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(table->log_prob.download(log_prob_out, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_frag_length_table_free(rpvg_hip_ctx * ctx, rpvg_hip_frag_table * table) {
    if (!table) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
    }
    delete table;
}

extern "C" int rpvg_hip_effective_lengths(rpvg_hip_ctx * ctx, double loc, double scale, double shape, const uint32_t * path_length, uint64_t n,
                                          double * out) {
    RPVG_REQUIRE(ctx && (n == 0 || (path_length && out)), "rpvg_hip_effective_lengths: NULL argument");
    if (n == 0) return RPVG_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<uint32_t> d_length;
    DeviceBuffer<double> d_out, d_lower;
    RPVG_HIP_CHECK(d_length.upload(path_length, n, st));
    RPVG_HIP_CHECK(d_out.alloc(n));
    if (const int rc = launchEffectiveLengths(st, loc, scale, shape, d_length.ptr, n, d_out.ptr, d_lower)) return rc;
    RPVG_HIP_CHECK(d_out.download(out, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_frag_length_eval(rpvg_hip_ctx * ctx, int what, const double * rows, uint64_t n, double * out) {
    RPVG_REQUIRE(ctx && (n == 0 || (rows && out)), "rpvg_hip_frag_length_eval: NULL argument");
    RPVG_REQUIRE(what >= 0 && what <= 2, "rpvg_hip_frag_length_eval: what = %d", what);
    RPVG_REQUIRE(n < (1ull << 32), "rpvg_hip_frag_length_eval: %llu rows exceed one call", static_cast<unsigned long long>(n));
    if (n == 0) return RPVG_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<double> d_rows, d_out;
    RPVG_HIP_CHECK(d_rows.upload(rows, n * 5, st));
    RPVG_HIP_CHECK(d_out.alloc(n));
    fragLengthEvalKernel<<<gridOf(n, 256), dim3(256), 0, st>>>(n, what, d_rows.ptr, gaussLegendre(), d_out.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_out.download(out, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

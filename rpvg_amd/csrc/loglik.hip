// The log-likelihood contraction over the group (haplotype / diplotype) matrices
// on the GPU (gfx950); group_build.hip builds the matrices.
//
// Takes over
//   read_counts * (noise + sum cols / g).array().log().matrix()
//                                            src/path_estimator.cpp:354-361,424-427,439,527-545
//
// The matrices are column-major (a wave walking the rows of one or two columns
// reads contiguous memory) with their rows ordered by class (count 1 first:
// partitionRowsKernel, group_build.hip), so that the contraction — FP64-issue
// bound, not HBM bound: a cluster's matrix is re-read from L2 by every request
// that touches it — replaces most logarithms by a running product (LogProduct).

#include "common.hpp"

using namespace rpvg_hip_detail;

namespace {

constexpr uint32_t kNoMember = 0xFFFFFFFFu;

// one wave per request
template <int WIDTH>
__global__ __launch_bounds__(256) void groupLoglikKernel(
    const uint32_t num_requests, const uint32_t * __restrict__ req_matrix, const uint32_t * __restrict__ req_members,
    const uint8_t * __restrict__ req_rowmax, const double divisor, const GroupMatricesView matrices, double * __restrict__ out) {
    __shared__ LogTableEntry lt[kLogTableSize];
    loadLogTable(lt);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (q >= num_requests) return;
    const GroupMatrix mat = matrices.matrix(req_matrix[q]);
    const uint64_t R = mat.R;
    const double * M = mat.values, * cnt = mat.row_count, * nz = mat.row_noise;
    const double * rm = req_rowmax && req_rowmax[q] ? mat.rowmax : nullptr;
    const double * col[WIDTH];
#pragma unroll
    for (int w = 0; w < WIDTH; ++w) {
        const uint32_t g = req_members[static_cast<uint64_t>(q) * WIDTH + w];
        col[w] = (g == kNoMember) ? nullptr : M + static_cast<uint64_t>(g) * R;
    }
    auto x = [&](const uint64_t i) {
        double v = nz[i];
#pragma unroll
        for (int w = 0; w < WIDTH; ++w)
            if (col[w]) v += col[w][i] / divisor;
        if (rm) v += rm[i] / divisor;
        return v;
    };
    const double acc = waveSumF64(sumCountLogs<uint64_t>(lt, cnt, x, 0, mat.fast_end, mat.mid_end, R, lane));
    if (lane == 0) out[q] = acc;
}

// Conditionals of the Gibbs sampler (src/path_estimator.cpp:527-545): request q fixes the other WIDTH-1 members of a
// group on its matrix and asks for the log-likelihood of every candidate column.  One wave per (request, 4 candidate
// columns): the base vector noise + sum(others)/g is formed once per row and shared by the four logs (same order
// of additions as the reference: noise, the others in slot order, then the candidate).
template <int WIDTH>
__global__ __launch_bounds__(256) void groupConditionalKernel(
    const uint32_t num_requests, const uint64_t num_items, const uint64_t * __restrict__ item_off,
    const uint64_t * __restrict__ out_off, const uint32_t * __restrict__ req_matrix,
    const uint32_t * __restrict__ req_others, const double divisor, const GroupMatricesView matrices, double * __restrict__ out) {
    constexpr int kCand = 4;
    __shared__ LogTableEntry lt[kLogTableSize];
    loadLogTable(lt);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t item = (blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (item >= num_items) return;
    uint32_t lo = 0, hi = num_requests - 1;  // last q with item_off[q] <= item
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (item_off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const uint32_t q = lo;
    const GroupMatrix mat = matrices.matrix(req_matrix[q]);
    const uint64_t R = mat.R;
    const uint32_t G = mat.G;
    const uint32_t k0 = static_cast<uint32_t>(item - item_off[q]) * kCand;
    const double * M = mat.values, * cnt = mat.row_count, * nz = mat.row_noise;
    const double * other[WIDTH > 1 ? WIDTH - 1 : 1];
#pragma unroll
    for (int w = 0; w + 1 < WIDTH; ++w) other[w] = M + static_cast<uint64_t>(req_others[static_cast<uint64_t>(q) * (WIDTH - 1) + w]) * R;
    const double * cand[kCand];
#pragma unroll
    for (int c = 0; c < kCand; ++c) cand[c] = M + static_cast<uint64_t>(min(k0 + c, G - 1)) * R;
    double acc[kCand] = {0.0, 0.0, 0.0, 0.0};
    LogProduct pr[kCand];
    const uint64_t fast_end = mat.fast_end, mid_end = mat.mid_end;
    auto x = [&](const uint64_t i, double (&xs)[kCand]) {
        double base = nz[i];
#pragma unroll
        for (int w = 0; w + 1 < WIDTH; ++w) base += other[w][i] / divisor;
#pragma unroll
        for (int c = 0; c < kCand; ++c) xs[c] = base + cand[c][i] / divisor;
    };
    sumCountLogsMulti<kCand, 64, uint64_t>(lt, cnt, x, 0, fast_end, mid_end, R, lane, pr, acc);
    if (mid_end) {
#pragma unroll
        for (int c = 0; c < kCand; ++c) acc[c] += pr[c].value(lt);
    }
#pragma unroll
    for (int c = 0; c < kCand; ++c) {
        const double total = waveSumF64(acc[c]);
        if (lane == 0 && k0 + c < G) out[out_off[q] + k0 + c] = total;
    }
}

__global__ void debugLogKernel(const uint64_t n, const double * __restrict__ x, double * __restrict__ out, const int use_table) {
    __shared__ LogTableEntry lt[kLogTableSize];
    loadLogTable(lt);
    __syncthreads();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < n) out[i] = use_table ? logPositive(x[i], lt) : logPositive(x[i]);
}

}  // namespace

extern "C" int rpvg_hip_debug_log(rpvg_hip_ctx * ctx, uint64_t n, const double * x, double * out, int32_t use_table) {
    RPVG_REQUIRE(ctx && x && out, "rpvg_hip_debug_log: NULL argument");
    if (n == 0) return RPVG_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    DeviceBuffer<double> d_x, d_out;
    RPVG_HIP_CHECK(d_x.upload(x, n, ctx->stream));
    RPVG_HIP_CHECK(d_out.alloc(n));
    debugLogKernel<<<dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(n, d_x.ptr, d_out.ptr, use_table);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_out.download(out, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_group_loglik(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_requests,
                                     const uint32_t * matrix, const uint32_t * members, uint32_t width, double divisor,
                                     const uint8_t * add_rowmax, double * out) {
    RPVG_REQUIRE(ctx && groups, "rpvg_hip_group_loglik: NULL argument");
    if (num_requests == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(matrix && members && out, "rpvg_hip_group_loglik: NULL request arrays");
    RPVG_REQUIRE(width >= 1 && width <= 8, "rpvg_hip_group_loglik: width %u outside [1, 8]", width);
    RPVG_REQUIRE(divisor > 0, "rpvg_hip_group_loglik: divisor must be positive");
    double evals = 0;
    for (uint32_t q = 0; q < num_requests; ++q) {
        RPVG_REQUIRE(matrix[q] < groups->num_matrices, "rpvg_hip_group_loglik: request %u refers to matrix %u of %u", q,
                     matrix[q], groups->num_matrices);
        for (uint32_t w = 0; w < width; ++w) {
            const uint32_t mem = members[static_cast<uint64_t>(q) * width + w];
            RPVG_REQUIRE(mem == kNoMember || mem < groups->h_num_cols[matrix[q]],
                         "rpvg_hip_group_loglik: request %u member %u >= %u columns", q, mem, groups->h_num_cols[matrix[q]]);
        }
        evals += static_cast<double>(groups->h_num_rows[matrix[q]]);
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(groups->waitCollapse(st));
    DeviceBuffer<uint32_t> d_matrix, d_members;
    DeviceBuffer<uint8_t> d_flag;
    DeviceBuffer<double> d_out;
    int span = ctx->spanBegin(FAM_H2D);
    RPVG_HIP_CHECK(d_matrix.upload(matrix, num_requests, st));
    RPVG_HIP_CHECK(d_members.upload(members, static_cast<size_t>(num_requests) * width, st));
    if (add_rowmax) RPVG_HIP_CHECK(d_flag.upload(add_rowmax, num_requests, st));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(num_requests) * (4 + 4 * width + (add_rowmax ? 1 : 0));
    RPVG_HIP_CHECK(d_out.alloc(num_requests));

    const uint32_t blocks = (num_requests + 3) / 4;
    span = ctx->spanBegin(FAM_LOGLIK);
#define RPVG_LAUNCH_LOGLIK(W)                                                                                              \
    groupLoglikKernel<W><<<dim3(blocks), dim3(256), 0, st>>>(num_requests, d_matrix.ptr, d_members.ptr, d_flag.ptr, divisor, groups->view(), d_out.ptr)
    switch (width) {
        case 1: RPVG_LAUNCH_LOGLIK(1); break;
        case 2: RPVG_LAUNCH_LOGLIK(2); break;
        case 3: RPVG_LAUNCH_LOGLIK(3); break;
        case 4: RPVG_LAUNCH_LOGLIK(4); break;
        case 5: RPVG_LAUNCH_LOGLIK(5); break;
        case 6: RPVG_LAUNCH_LOGLIK(6); break;
        case 7: RPVG_LAUNCH_LOGLIK(7); break;
        default: RPVG_LAUNCH_LOGLIK(8); break;
    }
#undef RPVG_LAUNCH_LOGLIK
    ctx->spanEnd(span);
    ctx->stats.loglik_launches += 1;
    ctx->stats.loglik_evals += evals;
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_out.download(out, st));
    RPVG_HIP_CHECK(waitStream(st));
    return groups->buildError(st);  // the matrices were built without a host sync
}

extern "C" int rpvg_hip_group_conditionals(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_requests,
                                           const uint32_t * matrix, const uint32_t * others, uint32_t width,
                                           double divisor, double * out) {
    RPVG_REQUIRE(ctx && groups, "rpvg_hip_group_conditionals: NULL argument");
    if (num_requests == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(matrix && out && (others || width == 1), "rpvg_hip_group_conditionals: NULL request arrays");
    RPVG_REQUIRE(width >= 1 && width <= 8, "rpvg_hip_group_conditionals: width %u outside [1, 8]", width);
    RPVG_REQUIRE(divisor > 0, "rpvg_hip_group_conditionals: divisor must be positive");
    std::vector<uint64_t> item_off(num_requests + 1, 0), out_off(num_requests + 1, 0);
    double evals = 0;
    for (uint32_t q = 0; q < num_requests; ++q) {
        RPVG_REQUIRE(matrix[q] < groups->num_matrices, "rpvg_hip_group_conditionals: request %u refers to matrix %u of %u",
                     q, matrix[q], groups->num_matrices);
        const uint32_t G = groups->h_num_cols[matrix[q]];
        for (uint32_t w = 0; w + 1 < width; ++w) {
            RPVG_REQUIRE(others[static_cast<uint64_t>(q) * (width - 1) + w] < G,
                         "rpvg_hip_group_conditionals: request %u member %u >= %u columns", q,
                         others[static_cast<uint64_t>(q) * (width - 1) + w], G);
        }
        item_off[q + 1] = item_off[q] + (G + 3) / 4;
        out_off[q + 1] = out_off[q] + G;
        evals += static_cast<double>(groups->h_num_rows[matrix[q]]) * G;
    }
    const uint64_t num_items = item_off[num_requests];

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(groups->waitCollapse(st));
    DeviceBuffer<uint32_t> d_matrix, d_others;
    DeviceBuffer<uint64_t> d_item_off, d_out_off;
    DeviceBuffer<double> d_out;
    int span = ctx->spanBegin(FAM_H2D);
    RPVG_HIP_CHECK(d_matrix.upload(matrix, num_requests, st));
    if (width > 1) RPVG_HIP_CHECK(d_others.upload(others, static_cast<size_t>(num_requests) * (width - 1), st));
    RPVG_HIP_CHECK(d_item_off.upload(item_off.data(), item_off.size(), st));
    RPVG_HIP_CHECK(d_out_off.upload(out_off.data(), out_off.size(), st));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(num_requests) * (4 + 4 * (width - 1) + 16);
    RPVG_HIP_CHECK(d_out.alloc(out_off[num_requests]));

    const uint64_t blocks = (num_items + 3) / 4;
    RPVG_REQUIRE(blocks <= 0x7fffffffull, "rpvg_hip_group_conditionals: %llu work items exceed one launch",
                 static_cast<unsigned long long>(num_items));
    span = ctx->spanBegin(FAM_LOGLIK);
#define RPVG_LAUNCH_COND(W)                                                                                                  \
    groupConditionalKernel<W><<<dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st>>>(                                    \
        num_requests, num_items, d_item_off.ptr, d_out_off.ptr, d_matrix.ptr, d_others.ptr, divisor, groups->view(), d_out.ptr)
    switch (width) {
        case 1: RPVG_LAUNCH_COND(1); break;
        case 2: RPVG_LAUNCH_COND(2); break;
        case 3: RPVG_LAUNCH_COND(3); break;
        case 4: RPVG_LAUNCH_COND(4); break;
        case 5: RPVG_LAUNCH_COND(5); break;
        case 6: RPVG_LAUNCH_COND(6); break;
        case 7: RPVG_LAUNCH_COND(7); break;
        default: RPVG_LAUNCH_COND(8); break;
    }
#undef RPVG_LAUNCH_COND
    ctx->spanEnd(span);
    ctx->stats.loglik_launches += 1;
    ctx->stats.loglik_evals += evals;
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_out.download(out, st));
    RPVG_HIP_CHECK(waitStream(st));
    return groups->buildError(st);  // the matrices were built without a host sync
}

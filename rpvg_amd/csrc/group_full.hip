// Full enumeration of the group (haplotype) posteriors on the GPU (gfx950): every multiset of group_size columns of a
// matrix, its log-likelihood, log frequencies and permutation count, and the normalisation — all on the device.
//
// Takes over
//   calculatePathGroupPosteriorsFull         src/path_estimator.cpp:332-377
//   Utils::numPermutations                   src/utils.hpp:95-117 (as a table indexed by the number of distinct members)
//
// Sets are identified by their rank in lexicographic order (the order of PathClusterEstimates::generateGroups): a
// non-decreasing m_1 .. m_g over G columns is the combination m_i + i - 1 of G + g - 1, and a rank maps to it through
// the combinatorial number system.  The host never lists members.
//
// Layout: one wave per (g-1)-prefix of a problem.  The sets that share a prefix are consecutive in lexicographic order
// (last member from the prefix's largest member to G - 1): the wave walks them in blocks of kFullCand candidates, and
// per row forms noise + sum(prefix)/g once for the block, the way groupConditionalKernel (loglik.hip) shares its base
// vector.  The order of additions is the reference's: noise, then the members in ascending order, each divided by g.
// A second kernel normalises each problem with a fixed-order reduction (maximum, then a fixed tree of exp(x - max)):
// two runs give the same bits.

#include "common.hpp"
#include "subset_full_plan.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace rpvg_hip_detail;

namespace {

constexpr int kFullCand = 4;            // candidate last members per pass over the rows
constexpr int kFullNormBlock = 256;     // threads of the per-problem normalisation

struct FullLogPerm {
    double v[8];
};

// C(n, k), k <= 8, for the values the enumeration takes: every one counts a subset of one problem's sets, at most
// RPVG_HIP_FULL_MAX_SETS, so the running product C(n - k + j - 1, j - 1) * (n - k + j) stays below 2^63.
__host__ __device__ inline uint64_t smallBinomial(const uint64_t n, const uint32_t k) {
    if (k > n) return 0;
    uint64_t r = 1;
    for (uint32_t j = 1; j <= k; ++j) r = r * (n - k + j) / j;
    return r;
}

// One wave per (problem, prefix).  log_perm[u - 1] = log(numPermutations) of a set with u distinct members.
template <int GS>
__global__ __launch_bounds__(256) void groupFullKernel(
    const uint32_t num_problems, const uint64_t num_items, const uint64_t * __restrict__ prefix_off,
    const uint64_t * __restrict__ set_off, const uint64_t * __restrict__ lf_off, const uint32_t * __restrict__ req_matrix,
    const double * __restrict__ log_freq, const FullLogPerm log_perm, const GroupMatricesView matrices, double * __restrict__ out) {
    constexpr int kPre = GS - 1;
    __shared__ LogTableEntry lt[kLogTableSize];
    loadLogTable(lt);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t item = (blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (item >= num_items) return;
    uint32_t lo = 0, hi = num_problems - 1;  // last q with prefix_off[q] <= item
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (prefix_off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const uint32_t q = lo;
    const GroupMatrix mat = matrices.matrix(req_matrix[q]);
    const uint64_t R = mat.R;
    const uint32_t G = mat.G;
    const double divisor = static_cast<double>(GS);

    // the prefix: combination of kPre out of G + kPre - 1 with rank `p` (lexicographic), members = element - position
    uint32_t pre[kPre > 0 ? kPre : 1];
    uint64_t p = item - prefix_off[q];
    {
        const uint64_t n = static_cast<uint64_t>(G) + kPre - 1;
        uint64_t x = 0;
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            for (; x < n; ++x) {
                const uint64_t c = smallBinomial(n - 1 - x, static_cast<uint32_t>(kPre - 1 - i));
                if (p < c) break;
                p -= c;
            }
            pre[i] = static_cast<uint32_t>(x) - i;
            ++x;
        }
    }
    const uint32_t last = kPre > 0 ? pre[kPre > 0 ? kPre - 1 : 0] : 0;

    // rank of the set (prefix, last): combination b_i = member_i + i of G + GS - 1
    uint64_t rank = 0;
    {
        const uint64_t n = static_cast<uint64_t>(G) + GS - 1;
        uint64_t x = 0;
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            const uint64_t b = static_cast<uint64_t>(i < kPre ? pre[i < kPre ? i : 0] : last) + i;
            for (; x < b; ++x) rank += smallBinomial(n - 1 - x, static_cast<uint32_t>(GS - 1 - i));
            ++x;
        }
    }
    uint32_t distinct = kPre > 0 ? 1 : 0;
#pragma unroll
    for (int i = 1; i < kPre; ++i) distinct += (pre[i] != pre[i - 1]);

    const double * M = mat.values, * cnt = mat.row_count, * nz = mat.row_noise;
    const double * lf = log_freq + lf_off[q];
    const double * prefix_col[kPre > 0 ? kPre : 1];
#pragma unroll
    for (int w = 0; w < kPre; ++w) prefix_col[w] = M + static_cast<uint64_t>(pre[w]) * R;
    const uint64_t fast_end = mat.fast_end, mid_end = mat.mid_end;
    double * dst = out + set_off[q] + rank;

    for (uint32_t k0 = last; k0 < G; k0 += kFullCand) {
        const double * cand[kFullCand];
#pragma unroll
        for (int c = 0; c < kFullCand; ++c) cand[c] = M + static_cast<uint64_t>(min(k0 + c, G - 1)) * R;
        double acc[kFullCand];
        LogProduct pr[kFullCand];
#pragma unroll
        for (int c = 0; c < kFullCand; ++c) acc[c] = 0.0;
        auto x = [&](const uint64_t i, double (&xs)[kFullCand]) {
            double base = nz[i];
#pragma unroll
            for (int w = 0; w < kPre; ++w) base += prefix_col[w][i] / divisor;
#pragma unroll
            for (int c = 0; c < kFullCand; ++c) xs[c] = base + cand[c][i] / divisor;
        };
        sumCountLogsMulti<kFullCand, 64, uint64_t>(lt, cnt, x, 0, fast_end, mid_end, R, lane, pr, acc);
        if (mid_end) {
#pragma unroll
            for (int c = 0; c < kFullCand; ++c) acc[c] += pr[c].value(lt);
        }
#pragma unroll
        for (int c = 0; c < kFullCand; ++c) {
            double v = waveSumF64(acc[c]);
            const uint32_t k = k0 + c;
            if (lane == 0 && k < G) {
                // + log frequency of every member in ascending order, + log(numPermutations) (src/path_estimator.cpp:363-369)
#pragma unroll
                for (int w = 0; w < kPre; ++w) v += lf[pre[w]];
                v += lf[k];
                const uint32_t u = distinct + ((kPre == 0 || k != last) ? 1u : 0u);
                v += log_perm.v[u - 1];
                dst[k - last] = v;
            }
        }
    }
}

// One workgroup per problem: x -> exp(x - log(sum exp x)), the sum as max + log(sum exp(x - max)) in a fixed order.
__global__ __launch_bounds__(kFullNormBlock) void groupFullNormaliseKernel(const uint64_t * __restrict__ set_off, double * __restrict__ x) {
    __shared__ double red[kFullNormBlock];
    const uint64_t begin = set_off[blockIdx.x], end = set_off[blockIdx.x + 1];
    const int t = threadIdx.x;
    double mx = -HUGE_VAL;
    for (uint64_t j = begin + t; j < end; j += kFullNormBlock) mx = fmax(mx, x[j]);
    red[t] = mx;
    __syncthreads();
    for (int s = kFullNormBlock / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    double sum = 0.0;
    for (uint64_t j = begin + t; j < end; j += kFullNormBlock) sum += exp(x[j] - mx);
    red[t] = sum;
    __syncthreads();
    for (int s = kFullNormBlock / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const double log_sum = mx + log(red[0]);
    for (uint64_t j = begin + t; j < end; j += kFullNormBlock) x[j] = exp(x[j] - log_sum);
}

}  // namespace

extern "C" uint64_t rpvg_hip_full_set_count(uint32_t columns, uint32_t group_size) {
    if (group_size == 0) return columns ? 1 : 0;
    // C(columns + group_size - 1, group_size), UINT64_MAX when it does not fit
    const unsigned __int128 n = static_cast<unsigned __int128>(columns) + group_size - 1;
    if (columns == 0) return 0;
    unsigned __int128 r = 1;
    for (uint32_t j = 1; j <= group_size; ++j) {
        r = r * (n - group_size + j) / j;
        if (r > static_cast<unsigned __int128>(UINT64_MAX)) return UINT64_MAX;
    }
    return static_cast<uint64_t>(r);
}

// One launch of the enumeration: the P problems matrix[0 .. P) with sets[0 .. P) sets each, their log frequencies back to back in
// log_freq, posteriors (normalised per problem) back to back in d_out, which holds the sum of `sets`.  Queued on the context's
// stream, which the caller has made wait for the matrices' collapse; `work` keeps the small device arrays until the stream is waited
// for.  rpvg_hip_group_full_posteriors and rpvg_hip_nested_full_subset_em (subset_full.hip) both go through here: one set of kernels,
// one order of additions.
int rpvg_hip_detail::queueGroupFullLaunch(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, const uint32_t * matrix, const uint32_t P,
                                          const uint64_t * sets, const uint32_t group_size, const double * log_freq, GroupFullLaunch & work,
                                          double * d_out) {
    hipStream_t st = ctx->stream;
    // log(numPermutations) by the number of distinct members: n! / (n - u + 1)! truncated to an integer (src/utils.hpp:95-117)
    FullLogPerm log_perm;
    for (uint32_t u = 1; u <= 8; ++u) {
        double perm = 1.0;
        if (group_size > 1 && u <= group_size) {
            perm = static_cast<double>(static_cast<uint32_t>(std::tgamma(group_size + 1) / std::tgamma(group_size - u + 2)));
        }
        log_perm.v[u - 1] = std::log(perm);
    }
    std::vector<uint64_t> prefix_off(P + 1, 0), set_off(P + 1, 0), lf_off(P, 0);
    uint64_t lf_count = 0;
    double evals = 0;
    for (uint32_t j = 0; j < P; ++j) {
        const uint32_t G = groups->h_num_cols[matrix[j]];
        prefix_off[j + 1] = prefix_off[j] + (G ? rpvg_hip_full_set_count(G, group_size - 1) : 0);
        set_off[j + 1] = set_off[j] + sets[j];
        lf_off[j] = lf_count;
        lf_count += G;
        evals += static_cast<double>(sets[j]) * static_cast<double>(groups->h_num_rows[matrix[j]]);
    }
    work.launch_sets = set_off[P];
    work.lf_count = lf_count;
    const uint64_t num_items = prefix_off[P];
    const uint64_t blocks = (num_items + 3) / 4;
    RPVG_REQUIRE(blocks <= 0x7fffffffull, "rpvg_hip_group_full_posteriors: %llu prefixes exceed one launch",
                 static_cast<unsigned long long>(num_items));
    int span = ctx->spanBegin(FAM_H2D);
    RPVG_HIP_CHECK(work.d_matrix.upload(matrix, P, st));
    RPVG_HIP_CHECK(work.d_prefix_off.upload(prefix_off.data(), P + 1, st));
    RPVG_HIP_CHECK(work.d_set_off.upload(set_off.data(), P + 1, st));
    RPVG_HIP_CHECK(work.d_lf_off.upload(lf_off.data(), P, st));
    RPVG_HIP_CHECK(work.d_lf.upload(log_freq, lf_count, st));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(P) * 28 + 8 + static_cast<double>(lf_count) * 8;
    if (num_items == 0) return RPVG_HIP_OK;
    span = ctx->spanBegin(FAM_LOGLIK);
#define RPVG_LAUNCH_FULL(W)                                                                                                     \
    groupFullKernel<W><<<dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st>>>(                                              \
        P, num_items, work.d_prefix_off.ptr, work.d_set_off.ptr, work.d_lf_off.ptr, work.d_matrix.ptr, work.d_lf.ptr, log_perm, \
        groups->view(), d_out)
    switch (group_size) {
        case 1: RPVG_LAUNCH_FULL(1); break;
        case 2: RPVG_LAUNCH_FULL(2); break;
        case 3: RPVG_LAUNCH_FULL(3); break;
        case 4: RPVG_LAUNCH_FULL(4); break;
        case 5: RPVG_LAUNCH_FULL(5); break;
        case 6: RPVG_LAUNCH_FULL(6); break;
        case 7: RPVG_LAUNCH_FULL(7); break;
        default: RPVG_LAUNCH_FULL(8); break;
    }
#undef RPVG_LAUNCH_FULL
    groupFullNormaliseKernel<<<dim3(P), dim3(kFullNormBlock), 0, st>>>(work.d_set_off.ptr, d_out);
    ctx->spanEnd(span);
    ctx->stats.loglik_launches += 2;
    ctx->stats.loglik_evals += evals;
    RPVG_HIP_CHECK(hipGetLastError());
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_group_full_posteriors(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_problems,
                                              const uint32_t * matrix, uint32_t group_size, const double * log_freq,
                                              double * posteriors) {
    RPVG_REQUIRE(ctx && groups, "rpvg_hip_group_full_posteriors: NULL argument");
    if (num_problems == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(matrix && log_freq && posteriors, "rpvg_hip_group_full_posteriors: NULL request arrays");
    RPVG_REQUIRE(group_size >= 1 && group_size <= 8, "rpvg_hip_group_full_posteriors: group size %u outside [1, 8]", group_size);
    std::vector<uint64_t> sets(num_problems);
    for (uint32_t q = 0; q < num_problems; ++q) {
        RPVG_REQUIRE(matrix[q] < groups->num_matrices, "rpvg_hip_group_full_posteriors: problem %u refers to matrix %u of %u", q,
                     matrix[q], groups->num_matrices);
        const uint32_t G = groups->h_num_cols[matrix[q]];
        sets[q] = rpvg_hip_full_set_count(G, group_size);
        if (sets[q] > RPVG_HIP_FULL_MAX_SETS) {
            rpvg_hip_detail::setError("rpvg_hip_group_full_posteriors: problem %u (matrix %u, %u columns) has more than %llu sets of %u",
                                      q, matrix[q], G, static_cast<unsigned long long>(RPVG_HIP_FULL_MAX_SETS), group_size);
            return RPVG_HIP_ERR_UNSUPPORTED;
        }
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(groups->waitCollapse(st));

    uint64_t out_first = 0, lf_first = 0;
    uint32_t first = 0;
    while (first < num_problems) {
        // the problems of one launch: up to kSetsPerLaunch outputs, a larger one alone
        const uint32_t end = rpvg_subset_full::chunkEnd(sets.data(), first, num_problems);
        uint64_t launch_sets = 0;
        for (uint32_t q = first; q < end; ++q) launch_sets += sets[q];
        GroupFullLaunch work;
        DeviceBuffer<double> d_out;
        RPVG_HIP_CHECK(d_out.alloc(launch_sets));
        const int rc = queueGroupFullLaunch(ctx, groups, matrix + first, end - first, sets.data() + first, group_size, log_freq + lf_first, work, d_out.ptr);
        if (rc != RPVG_HIP_OK) return rc;
        if (launch_sets) RPVG_HIP_CHECK(d_out.download(posteriors + out_first, st));
        RPVG_HIP_CHECK(waitStream(st));  // the buffers of this launch go back to the pool on the next round
        out_first += launch_sets;
        lf_first += work.lf_count;
        first = end;
    }
    return groups->buildError(st);  // the matrices were built without a host sync
}

// Weighted minimum path cover on the GPU (gfx950): the greedy set cover of
// MinimumPathAbundanceEstimator (`-i strains`).
//
// Takes over, per cluster,
//   the cover matrix / path weights set-up      src/path_abundance_estimator.cpp:233-257
//   weightedMinimumPathCover                    src/path_abundance_estimator.cpp:297-340
// ONE workgroup per listed cluster runs all greedy rounds: per round every still-uncovered row adds its read
// count to the paths it contains (integers in FP64: exact in any order), the block picks the path with
// the largest covered-reads / weight (first index among equals, as the reference's ascending scan
// does), and the rows containing it become covered.  Integer/compare work on the sparse rows; the only
// floating point is the path weight  -sum_i count_i log(prob_ij)  and one division per path per round.
//
// The weight of a path is added up in ASCENDING ROW ORDER, as the reference adds it (:239-248): all threads compute the
// terms count_i log(prob_ij) of a window of entries, then one wavefront adds them to the weights row by row.  A weight is
// therefore a function of the path's (row, count, probability) terms alone — not of the place of the path in the rows'
// entry lists, of the lanes that meet, or of timing: two paths with the same terms ("twins": haplotype paths the reads
// cannot tell apart) get the same bits and tie, and the tie goes to the lower index as in the reference.
// The chosen paths are kept as a bit per path and written out in ascending order by a prefix sum (:337).

#include "common.hpp"
#include "cover_plan.hpp"
#include "cover_terms.hpp"

#include <algorithm>
#include <vector>

using namespace rpvg_hip_detail;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxPaths = rpvg_cover::kWorkgroupMaxPaths;  // two vectors of doubles per path in 150 KiB of LDS

// covered: one byte per row of every LISTED problem (problem p's rows from covered_off[p]): a cluster listed twice is two
// independent problems.
__global__ __launch_bounds__(kBlock) void minPathCoverKernel(
    const uint32_t num_problems, const uint32_t * __restrict__ prob_cluster, const uint64_t * __restrict__ cluster_row_off,
    const uint64_t * __restrict__ cluster_path_off, const uint64_t * __restrict__ row_ent_off,
    const uint32_t * __restrict__ ent_path, const double * __restrict__ ent_prob, const double * __restrict__ row_count,
    const double * __restrict__ row_noise, const uint64_t * __restrict__ out_off, const uint64_t * __restrict__ covered_off,
    uint8_t * __restrict__ covered_all, uint32_t * __restrict__ cover_out, uint32_t * __restrict__ cover_size) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red_val[kBlock / 64];
    __shared__ uint32_t red_idx[kBlock / 64];
    __shared__ uint32_t best_shared;
    __shared__ uint32_t scan_scratch[kBlock / 64];
    __shared__ uint32_t chosen[kMaxPaths / 32];  // bit j: path j is in the cover
    // a batch of kBlock rows (entry offsets from the batch's first entry, counts) and a window of kBlock of its entries
    __shared__ uint32_t batch_off[kBlock + 1];
    __shared__ double batch_count[kBlock];
    __shared__ double win_term[kBlock];
    __shared__ uint32_t win_path[kBlock];
    __shared__ uint8_t win_row[kBlock];
    static_assert(kMaxPaths % 32 == 0 && kBlock <= 256, "chosen is whole words; win_row holds a row of the batch in a byte");
    const uint32_t p = blockIdx.x;
    if (p >= num_problems) return;
    const uint32_t k = prob_cluster[p];
    const uint64_t r0 = cluster_row_off[k], r1 = cluster_row_off[k + 1];
    const uint32_t N = static_cast<uint32_t>(cluster_path_off[k + 1] - cluster_path_off[k]);
    double * weights = reinterpret_cast<double *>(smem_raw);  // [N]
    double * cov = weights + N;                                // [N]
    uint8_t * covered = covered_all + covered_off[p];          // [r1 - r0]
    uint32_t * out = cover_out + out_off[p];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t num_words = (N + 31) >> 5;

    if (N == 1) {  // src/path_abundance_estimator.cpp:302-305
        if (threadIdx.x == 0) {
            out[0] = 0;
            cover_size[p] = 1;
        }
        return;
    }

    for (uint32_t j = threadIdx.x; j < N; j += kBlock) weights[j] = 0.0;
    for (uint32_t w = threadIdx.x; w < num_words; w += kBlock) chosen[w] = 0;
    // path weights (:240-257); rows whose noise probability is 1 carry no reads for the cover
    for (uint64_t rb = r0; rb < r1; rb += kBlock) {
        const uint32_t batch_rows = (r1 - rb < kBlock) ? static_cast<uint32_t>(r1 - rb) : kBlock;
        const uint64_t e_first = row_ent_off[rb];
        __syncthreads();  // (the previous batch is done with batch_off / batch_count; first batch: weights are zero)
        if (threadIdx.x < batch_rows) {
            const uint64_t r = rb + threadIdx.x;
            const double c = coverRowCount(row_count[r], row_noise[r]);
            covered[r - r0] = (c > 0.0) ? 0 : 1;
            batch_count[threadIdx.x] = c;
            batch_off[threadIdx.x + 1] = static_cast<uint32_t>(row_ent_off[r + 1] - e_first);
        }
        if (threadIdx.x == 0) batch_off[0] = 0;
        __syncthreads();
        const uint32_t batch_entries = batch_off[batch_rows];
        for (uint32_t w0 = 0; w0 < batch_entries; w0 += kBlock) {
            const uint32_t t = w0 + threadIdx.x;
            if (t < batch_entries) {
                // the row of entry t: the last one that starts at or before it (rows without entries never qualify)
                uint32_t lo = 0, hi = batch_rows;  // batch_off[lo] <= t < batch_off[hi]
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (batch_off[mid] <= t) lo = mid; else hi = mid;
                }
                win_row[threadIdx.x] = static_cast<uint8_t>(lo);
                win_path[threadIdx.x] = ent_path[e_first + t];
                win_term[threadIdx.x] = coverTerm(ent_prob[e_first + t], batch_count[lo]);
            }
            __syncthreads();
            if (wave == 0) {
                // one wavefront, one row per step: a path receives at most one term per step (a row holds a path once; the
                // addition is atomic all the same, so that a row that broke that rule would lose no term)
                const uint32_t win_entries = (batch_entries - w0 < kBlock) ? batch_entries - w0 : kBlock;
                for (uint32_t q = 0; q < win_entries; q += 64) {
                    const uint32_t i = q + lane;
                    const bool valid = i < win_entries;
                    const uint32_t row = valid ? win_row[i] : 0xFFFFFFFFu;
                    const uint32_t path = valid ? win_path[i] : 0;
                    const double term = valid ? win_term[i] : 0.0;
                    const uint32_t first_row = win_row[q], last_row = win_row[(q + 63 < win_entries) ? q + 63 : win_entries - 1];
                    for (uint32_t rr = first_row; rr <= last_row; ++rr) {
                        if (row == rr) atomicAdd(&weights[path], term);
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < N; j += kBlock) weights[j] *= -1.0;

    uint32_t n_cover = 0;
    while (true) {
        for (uint32_t j = threadIdx.x; j < N; j += kBlock) cov[j] = 0.0;
        __syncthreads();
        for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
            if (!covered[r - r0]) {
                const double c = row_count[r];
                for (uint64_t e = row_ent_off[r]; e < row_ent_off[r + 1]; ++e) atomicAdd(&cov[ent_path[e]], c);
            }
        }
        __syncthreads();
        // first index with the largest positive covered / weight
        double best_val = 0.0;
        uint32_t best_idx = 0xFFFFFFFFu;
        for (uint32_t j = threadIdx.x; j < N; j += kBlock) {
            const double v = cov[j] / weights[j];
            if (v > best_val) {
                best_val = v;
                best_idx = j;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(best_val, d, 64);
            const uint32_t oi = __shfl_xor(best_idx, d, 64);
            if (ov > best_val || (ov == best_val && oi < best_idx)) {
                best_val = ov;
                best_idx = oi;
            }
        }
        if (lane == 0) {
            red_val[wave] = best_val;
            red_idx[wave] = best_idx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double bv = red_val[0];
            uint32_t bi = red_idx[0];
            for (int w = 1; w < kBlock / 64; ++w) {
                if (red_val[w] > bv || (red_val[w] == bv && red_idx[w] < bi)) {
                    bv = red_val[w];
                    bi = red_idx[w];
                }
            }
            best_shared = (bv > 0.0) ? bi : 0xFFFFFFFFu;
            if (bv > 0.0) chosen[bi >> 5] |= 1u << (bi & 31);
        }
        __syncthreads();
        const uint32_t best = best_shared;
        if (best == 0xFFFFFFFFu) break;  // nothing left to cover
        ++n_cover;
        for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
            if (!covered[r - r0]) {
                bool hit = false;
                for (uint64_t e = row_ent_off[r]; e < row_ent_off[r + 1]; ++e) hit = hit || (ent_path[e] == best);
                if (hit) covered[r - r0] = 1;
            }
        }
        __syncthreads();
    }
    // ascending order (:337): the set bits of `chosen`, each word's place from a prefix sum of the words' bit counts
    uint32_t written = 0;
    for (uint32_t w0 = 0; w0 < num_words; w0 += kBlock) {
        const uint32_t w = w0 + threadIdx.x;
        uint32_t bits = (w < num_words) ? chosen[w] : 0;
        uint32_t total;
        uint32_t at = written + blockExclusiveSum<kBlock>(static_cast<uint32_t>(__popc(bits)), total, scan_scratch);
        while (bits) {
            out[at++] = (w << 5) + static_cast<uint32_t>(__ffs(static_cast<int>(bits)) - 1);
            bits &= bits - 1;
        }
        written += total;
    }
    if (threadIdx.x == 0) cover_size[p] = n_cover;
}

}  // namespace

// The workgroup route of the listed clusters: validation, one launch, the covers on the host.  The caller holds the context's mutex
// (rpvg_hip_min_path_cover, and rpvg_hip_min_path_cover_any for the clusters it leaves on this route: path_cover_grid.hip).
int rpvg_hip_detail::minPathCoverWorkgroups(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters, const uint32_t * clusters,
                                            const uint64_t * cover_off, uint32_t * cover, uint32_t * cover_size) {
    RPVG_REQUIRE(clusters && cover_off && cover && cover_size, "rpvg_hip_min_path_cover: NULL argument");
    uint32_t max_paths = 0;
    std::vector<uint64_t> covered_off(num_clusters + 1, 0);  // the rows of the listed problems, one after the other
    for (uint32_t i = 0; i < num_clusters; ++i) {
        const uint32_t k = clusters[i];
        RPVG_REQUIRE(k < batch->num_clusters, "rpvg_hip_min_path_cover: cluster %u of %u", k, batch->num_clusters);
        const uint64_t N = batch->h_cluster_path_off[k + 1] - batch->h_cluster_path_off[k];
        RPVG_REQUIRE(batch->h_cluster_row_off[k + 1] > batch->h_cluster_row_off[k] && N > 0, "rpvg_hip_min_path_cover: cluster %u is empty", k);
        RPVG_REQUIRE(cover_off[i + 1] - cover_off[i] >= N, "rpvg_hip_min_path_cover: output range of cluster %u is smaller than its %llu paths", k,
                     static_cast<unsigned long long>(N));
        max_paths = std::max<uint32_t>(max_paths, static_cast<uint32_t>(std::min<uint64_t>(N, UINT32_MAX)));
        covered_off[i + 1] = covered_off[i] + (batch->h_cluster_row_off[k + 1] - batch->h_cluster_row_off[k]);
    }
    RPVG_REQUIRE(max_paths <= kMaxPaths, "rpvg_hip_min_path_cover: a cluster with %u paths does not fit the LDS-resident weight vectors (at most %u)",
                 max_paths, kMaxPaths);
    const size_t lds = (static_cast<size_t>(max_paths) * 16 + 15) & ~static_cast<size_t>(15);

    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<uint32_t> d_clusters, d_cover, d_size;
    DeviceBuffer<uint64_t> d_off, d_covered_off;
    DeviceBuffer<uint8_t> d_covered;
    RPVG_HIP_CHECK(d_clusters.upload(clusters, num_clusters, st));
    RPVG_HIP_CHECK(d_off.upload(cover_off, num_clusters + 1, st));
    RPVG_HIP_CHECK(d_cover.alloc(cover_off[num_clusters]));
    RPVG_HIP_CHECK(d_size.alloc(num_clusters));
    RPVG_HIP_CHECK(d_covered_off.upload(covered_off.data(), num_clusters + 1, st));
    RPVG_HIP_CHECK(d_covered.alloc(covered_off[num_clusters]));
    hipFuncAttributes attr;
    RPVG_HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&minPathCoverKernel)));
    if (lds + attr.sharedSizeBytes > 64 * 1024) {  // (the staging arrays are static LDS)
        RPVG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&minPathCoverKernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    }
    const int span = ctx->spanBegin(FAM_BUILD);
    minPathCoverKernel<<<dim3(num_clusters), dim3(kBlock), lds, st>>>(
        num_clusters, d_clusters.ptr, batch->cluster_row_off.ptr, batch->cluster_path_off.ptr, batch->row_ent_off.ptr,
        batch->ent_path.ptr, batch->ent_prob.ptr, batch->row_count.ptr, batch->row_noise.ptr, d_off.ptr, d_covered_off.ptr,
        d_covered.ptr, d_cover.ptr, d_size.ptr);
    ctx->spanEnd(span);
    ctx->stats.build_launches += 1;
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_cover.download(cover, st));
    RPVG_HIP_CHECK(d_size.download(cover_size, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_min_path_cover(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters,
                                       const uint32_t * clusters, const uint64_t * cover_off, uint32_t * cover,
                                       uint32_t * cover_size) {
    RPVG_REQUIRE(ctx && batch, "rpvg_hip_min_path_cover: NULL argument");
    if (num_clusters == 0) return RPVG_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    return minPathCoverWorkgroups(ctx, batch, num_clusters, clusters, cover_off, cover, cover_size);
}

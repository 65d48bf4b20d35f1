// path_table.hip — the PathInfo of every path of a run resident on the GPU, read in the index's cluster order
// (interface include/rpvg_index.h).
//
// Takes over   the path side of a batch that starts from fragments: PathInfo::group_id and ::source_ids permuted into the
//              clusters of the index (the caller's loop, src/main.cpp:855-887), then the haplotype columns of path_sources.hip
//              group_name_index of `-i transcripts --path-info`          src/main.cpp:853-887
//              the collapsed PathInfo of every name group                src/main.cpp:909-951
//
// Path side    path_group_id is a gather by cluster_paths.  The source-id lists are ragged: lengths by cluster_paths, an
//              exclusive scan, then one wavefront per path copies its list (lanes stride over a list longer than 64).  The
//              gathered arrays are what rpvg_hip_batch_upload would have copied, so reservePathSources /
//              queuePathSourceKernels / finishPathSources form the columns unchanged.
// Name groups  the local group of a path is the rank of its name's first appearance along the cluster.  Three routes by
//              the cluster's size, all exact and all a function of the input alone (no atomic's arrival order, no id value
//              enters a result; the atomics only collect the clusters of the second route, each of which is independent):
//                <= 64 paths     one wavefront: every lane finds the earliest lane with its id by a loop of lane reads, the
//                                heads are a 64-bit ballot, the group is popcount(heads below the head's lane);
//                <= 4 096 paths  one workgroup: bitonic sort of (name_id, position) in LDS, the head of a run by binary
//                                search, a scan of the head flags over the positions;
//                beyond          global memory: stable radix sort of (cluster, name_id) with the positions as values, a max-scan
//                                for the run heads, a sum-scan of the head flags.
// Collapsed    the members of every group in ascending position (stable radix sort by group), one thread per group: 64-bit integer
// paths        sums, the effective-length sum added in member order with mulRounded / addRounded (common.hpp: a rounded product, then a
//              rounded sum — HIP's __dmul_rn / __dadd_rn are plain operators that hipcc contracts into a fused multiply-add), as
//              the reference's loop does.
// No kernel allocates; every array is sized by P, K, S or G.

#include "device_algos.hpp"
#include "path_table.hpp"
#include "table_kit.hpp"

using namespace rpvg_hip_detail;

namespace {

constexpr uint32_t kWavePaths = 64;    // name groups: clusters of at most that many paths take one wavefront
constexpr uint32_t kLdsPaths = 4096;   // ... one workgroup with 48 KiB of LDS (keys 32 KiB, first positions 16 KiB)
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr uint32_t kLdsGrid = 256;     // workgroups that walk the list of the second route

// bad = min over the offending paths (table_kit.hpp)
enum TableBad { kBadOffsets = 1, kBadEnd = 2 };
__global__ void validateTableKernel(const uint32_t num_paths, const uint64_t num_sources, const uint64_t * __restrict__ source_off,
                                    unsigned long long * __restrict__ bad) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= num_paths) return;
    int why = 0;
    if (source_off[p] > source_off[p + 1] || source_off[p + 1] > num_sources || (p == 0 && source_off[0] != 0)) why = kBadOffsets;
    else if (p + 1 == num_paths && source_off[num_paths] != num_sources) why = kBadEnd;
    if (why) reportOffender(bad, p, why);
}

template <typename T>
__global__ void gatherByClusterPathKernel(const uint32_t num_paths, const uint32_t * __restrict__ cluster_paths, const T * __restrict__ by_global_path,
                                          T * __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < num_paths) out[i] = by_global_path[cluster_paths[i]];
}

// lengths of the source-id lists in cluster order; cell P is 0 (the scan turns the P + 1 cells into offsets)
__global__ void sourceLengthsKernel(const uint32_t num_paths, const uint32_t * __restrict__ cluster_paths, const uint64_t * __restrict__ source_off,
                                    uint64_t * __restrict__ length) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > num_paths) return;
    uint64_t n = 0;
    if (i < num_paths) {
        const uint32_t g = cluster_paths[i];
        n = source_off[g + 1] - source_off[g];
    }
    length[i] = n;
}

// one wavefront per path: its list from the table's place to the place of the path in cluster order
__global__ __launch_bounds__(kBlock) void gatherSourcesKernel(const uint32_t num_paths, const uint32_t * __restrict__ cluster_paths,
                                                              const uint64_t * __restrict__ source_off, const uint32_t * __restrict__ source_id,
                                                              const uint64_t * __restrict__ out_off, const uint64_t num_sources,
                                                              uint32_t * __restrict__ out) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= num_paths) return;
    const uint32_t g = cluster_paths[i];
    const uint64_t from = source_off[g], n = source_off[g + 1] - from, to = out_off[i];
    if (to + n > num_sources) return;  // (cluster_paths is a permutation: cannot happen)
    for (uint64_t j = lane; j < n; j += 64) out[to + j] = source_id[from + j];
}

__global__ void clusterSourceOffKernel(const uint32_t num_clusters, const uint64_t * __restrict__ cluster_path_off, const uint64_t * __restrict__ path_source_off,
                                       uint64_t * __restrict__ cluster_src_off) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= num_clusters) cluster_src_off[k] = path_source_off[cluster_path_off[k]];
}

// ---- name groups ---------------------------------------------------------------------------------------------------------
struct GroupArgs {
    uint32_t num_clusters, num_paths;
    const uint64_t * cluster_path_off;  // [K+1]
    const uint32_t * cluster_paths;     // [P]
    const uint32_t * name_id;           // [P] by global path
    uint32_t * path_group;              // [P] cluster order
    uint32_t * group_count;             // [K+1], cell K = 0
    uint32_t * mid_list;                // [K] clusters of the workgroup route
    uint32_t * counters;                // [0] length of mid_list, [1] any cluster beyond LDS
};

// a wavefront per cluster; larger clusters are left to the other routes
__global__ __launch_bounds__(kBlock) void waveGroupsKernel(const GroupArgs a) {
    const uint32_t k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.num_clusters) return;
    const uint64_t p0 = a.cluster_path_off[k];
    const uint64_t N64 = a.cluster_path_off[k + 1] - p0;
    if (N64 > kWavePaths) {
        if (lane == 0) {
            if (N64 <= kLdsPaths) a.mid_list[atomicAdd(&a.counters[0], 1u)] = k;
            else a.counters[1] = 1u;
        }
        return;
    }
    const uint32_t N = static_cast<uint32_t>(N64);
    const uint32_t id = lane < N ? a.name_id[a.cluster_paths[p0 + lane]] : 0u;
    uint32_t first = lane;
    for (uint32_t j = 0; j < N; ++j) {
        const uint32_t other = __shfl(id, static_cast<int>(j), 64);
        if (other == id && j < first) first = j;
    }
    const unsigned long long heads = __ballot(lane < N && first == lane);
    if (lane < N) a.path_group[p0 + lane] = __popcll(heads & ((1ull << first) - 1ull));
    if (lane == 0) a.group_count[k] = __popcll(heads);
}

// a workgroup per cluster of the list: sort of (name_id, position) in LDS
__global__ __launch_bounds__(kBlock) void ldsGroupsKernel(const GroupArgs a) {
    __shared__ unsigned long long s_key[kLdsPaths];
    __shared__ uint32_t s_first[kLdsPaths];
    __shared__ uint32_t s_scan[kWavesPerBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t listed = min(a.counters[0], a.num_clusters);
    for (uint32_t turn = blockIdx.x; turn < listed; turn += gridDim.x) {
        __syncthreads();  // (the LDS of the cluster before)
        const uint32_t k = a.mid_list[turn];
        if (k >= a.num_clusters) continue;
        const uint64_t p0 = a.cluster_path_off[k];
        const uint64_t N64 = a.cluster_path_off[k + 1] - p0;
        if (N64 > kLdsPaths) continue;  // (not listed by waveGroupsKernel)
        const uint32_t N = static_cast<uint32_t>(N64);
        uint32_t M = 64;
        while (M < N) M <<= 1;
        for (uint32_t i = tid; i < M; i += kBlock) {
            s_key[i] = i < N ? ((static_cast<unsigned long long>(a.name_id[a.cluster_paths[p0 + i]]) << 32) | i) : ~0ull;
        }
        for (uint32_t size = 2; size <= M; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (uint32_t t = tid; t < M; t += kBlock) {
                    const uint32_t partner = t ^ stride;
                    if (partner > t) {
                        const unsigned long long x = s_key[t], y = s_key[partner];
                        const bool ascending = (t & size) == 0;
                        if ((x > y) == ascending) {
                            s_key[t] = y;
                            s_key[partner] = x;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // the first position of every path's name: the low half of the first key of its run
        for (uint32_t t = tid; t < N; t += kBlock) {
            const unsigned long long key = s_key[t], target = key & 0xffffffff00000000ull;
            uint32_t lo = 0, hi = t;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_key[mid] < target) lo = mid + 1;
                else hi = mid;
            }
            s_first[static_cast<uint32_t>(key)] = static_cast<uint32_t>(s_key[lo]);
        }
        __syncthreads();
        uint32_t * const s_rank = reinterpret_cast<uint32_t *>(s_key);  // (the keys are done with)
        uint32_t run = 0;
        for (uint32_t c0 = 0; c0 < N; c0 += kBlock) {
            const uint32_t pos = c0 + tid;
            const uint32_t head = (pos < N && s_first[pos] == pos) ? 1u : 0u;
            uint32_t total;
            const uint32_t before = blockExclusiveSum<kBlock>(head, total, s_scan);
            if (pos < N) s_rank[pos] = run + before;
            run += total;
        }
        __syncthreads();
        for (uint32_t pos = tid; pos < N; pos += kBlock) a.path_group[p0 + pos] = s_rank[s_first[pos]];
        if (tid == 0) a.group_count[k] = run;
    }
}

// the cluster of every position of cluster_paths: the last k with cluster_path_off[k] <= i
__global__ void positionClusterKernel(const uint32_t num_paths, const uint32_t num_clusters, const uint64_t * __restrict__ cluster_path_off,
                                      uint32_t * __restrict__ position_cluster) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_paths) return;
    uint32_t lo = 0, hi = num_clusters;  // first k with off[k] > i, in (0, K]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cluster_path_off[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    position_cluster[i] = lo - 1;
}

__global__ void globalKeysKernel(const uint32_t num_paths, const uint32_t * __restrict__ position_cluster, const uint32_t * __restrict__ cluster_paths,
                                 const uint32_t * __restrict__ name_id, unsigned long long * __restrict__ key, uint32_t * __restrict__ position) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_paths) return;
    key[i] = (static_cast<unsigned long long>(position_cluster[i]) << 32) | name_id[cluster_paths[i]];
    position[i] = i;
}

template <typename Key>
__global__ void runHeadKernel(const uint32_t n, const Key * __restrict__ key_sorted, uint32_t * __restrict__ head_or_zero) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) head_or_zero[j] = (j > 0 && key_sorted[j] != key_sorted[j - 1]) ? j : 0u;
}

__global__ void firstPositionKernel(const uint32_t n, const uint32_t * __restrict__ position_sorted, const uint32_t * __restrict__ run_head,
                                    uint32_t * __restrict__ first_position) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) first_position[position_sorted[j]] = position_sorted[run_head[j]];
}

__global__ void headFlagKernel(const uint32_t n, const uint32_t * __restrict__ first_position, uint32_t * __restrict__ is_head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) is_head[i] = (i < n && first_position[i] == i) ? 1u : 0u;
}

// the results of the global route for the clusters beyond LDS (the other clusters have theirs)
__global__ void globalGroupsKernel(const GroupArgs a, const uint32_t * __restrict__ position_cluster, const uint32_t * __restrict__ first_position,
                                   const uint32_t * __restrict__ head_rank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_paths) return;
    const uint32_t k = position_cluster[i];
    const uint64_t p0 = a.cluster_path_off[k], p1 = a.cluster_path_off[k + 1];
    if (p1 - p0 <= kLdsPaths) return;
    a.path_group[i] = head_rank[first_position[i]] - head_rank[p0];
    if (i == p0) a.group_count[k] = head_rank[p1] - head_rank[p0];
}

// ---- collapsed paths -----------------------------------------------------------------------------------------------------
__global__ void groupKeyKernel(const uint32_t num_paths, const uint32_t * __restrict__ position_cluster, const uint64_t * __restrict__ cluster_group_off,
                               const uint32_t * __restrict__ path_group, uint32_t * __restrict__ key, uint32_t * __restrict__ position) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_paths) return;
    key[i] = static_cast<uint32_t>(cluster_group_off[position_cluster[i]]) + path_group[i];
    position[i] = i;
}

// member_off[g] = the first cell of group g among the sorted members; every group has a member
__global__ void groupStartKernel(const uint32_t num_paths, const uint64_t num_groups, const uint32_t * __restrict__ key_sorted,
                                 uint32_t * __restrict__ member_off) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > num_paths) return;
    if (j == num_paths) {
        member_off[num_groups] = num_paths;
    } else if ((j == 0 || key_sorted[j] != key_sorted[j - 1]) && key_sorted[j] < num_groups) {
        member_off[key_sorted[j]] = j;
    }
}

enum GroupBad { kBadZeroCount = 1, kBadCountSum = 2, kBadLength = 3 };

struct CollapseArgs {
    uint64_t num_groups;
    uint32_t num_paths;
    const uint32_t * member_off;     // [G+1]
    const uint32_t * member;         // [P] positions in cluster order, ascending within a group
    const uint32_t * cluster_paths;  // [P]
    const uint32_t * name_id, * group_id, * source_count, * length;  // by global path
    const double * effective_length;
    uint32_t * out_first_path, * out_name_id, * out_group_id, * out_source_count, * out_length;  // [G]
    double * out_effective_length;
    unsigned long long * bad;        // min over the offending groups (table_kit.hpp)
};

// one thread per group: src/main.cpp:914-948 over the members in their order
__global__ __launch_bounds__(kBlock) void collapseGroupsKernel(const CollapseArgs a) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (g >= a.num_groups) return;
    const uint32_t j0 = a.member_off[g], j1 = a.member_off[g + 1];
    if (j0 >= j1 || j1 > a.num_paths) return;  // (every group has a member)
    unsigned long long count_sum = 0, length_sum = 0;
    double eff_sum = 0.0;
    int why = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t path = a.cluster_paths[a.member[j]];
        const uint32_t sc = a.source_count[path];
        if (sc == 0) why = kBadZeroCount;
        count_sum += sc;
        length_sum += static_cast<unsigned long long>(a.length[path]) * sc;
        const double term = mulRounded(a.effective_length[path], static_cast<double>(sc));
        eff_sum = (j == j0) ? term : addRounded(eff_sum, term);
    }
    if (!why && (count_sum > 0xffffffffull || count_sum == 0)) why = count_sum ? kBadCountSum : kBadZeroCount;
    double mean_length = 0.0;
    if (!why) {
        mean_length = round(__ddiv_rn(static_cast<double>(length_sum), static_cast<double>(count_sum)));  // half away from zero
        if (!(mean_length <= 4294967295.0)) why = kBadLength;
    }
    if (why) {
        reportOffender(a.bad, g, why);
        return;
    }
    const uint32_t first = a.cluster_paths[a.member[j0]];
    a.out_first_path[g] = first;
    a.out_name_id[g] = a.name_id[first];
    a.out_group_id[g] = a.group_id[first];
    a.out_source_count[g] = static_cast<uint32_t>(count_sum);
    a.out_length[g] = static_cast<uint32_t>(mean_length);
    a.out_effective_length[g] = __ddiv_rn(eff_sum, static_cast<double>(count_sum));
}

int bitsFor(uint64_t values) {  // bits that hold 0 .. values - 1
    int bits = 1;
    while (bits < 64 && (values - 1) >> bits) ++bits;
    return bits;
}

}  // namespace

namespace rpvg_hip_detail {

int attachPathSide(rpvg_hip_ctx * ctx, rpvg_hip_batch * b, const uint32_t * d_row_count_u32, const rpvg_hip_align_index * index,
                   const rpvg_hip_path_table * table) {
    AlignIndexParts ix;
    RPVG_REQUIRE(alignIndexParts(index, ix), "rpvg_hip_read_rows_to_batch_with_paths: the index is not finished");
    const uint32_t K = ix.num_clusters, P = ix.num_paths;
    RPVG_REQUIRE(table->num_paths == P, "rpvg_hip_read_rows_to_batch_with_paths: the table has %u paths, the index %u", table->num_paths, P);
    RPVG_REQUIRE(b->num_clusters == K && b->h_cluster_path_off == *ix.h_cluster_path_off,
                 "rpvg_hip_read_rows_to_batch_with_paths: the rows are not those of the index's clusters (collapsed rows have no path side)");
    hipStream_t st = ctx->stream;
    const uint64_t S = table->has_sources ? table->num_sources : 0;
    const bool columns = K > 0 && P > 0 && S > 0 && S <= 0xfffffff0ull;
    PathSourcesPending pending;
    DeviceBuffer<double> d_totals;
    DeviceBuffer<uint64_t> lengths;
    SpanScope span(ctx, FAM_BUILD);
    if (columns) {
        RPVG_HIP_CHECK(reservePathSources(b, K, P, S, pending));
    } else {
        RPVG_HIP_CHECK(b->path_group_id.alloc(P));
    }
    if (P) {
        gatherByClusterPathKernel<uint32_t><<<gridFor(P), dim3(kBlock), 0, st>>>(P, ix.cluster_paths, table->group_id.ptr, b->path_group_id.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
    }
    if (columns) {
        RPVG_HIP_CHECK(lengths.alloc(static_cast<size_t>(P) + 1));
        sourceLengthsKernel<<<gridFor(static_cast<uint64_t>(P) + 1), dim3(kBlock), 0, st>>>(P, ix.cluster_paths, table->source_off.ptr, lengths.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = exclusiveSum(st, lengths.ptr, pending.d_path_source_off.ptr, static_cast<uint64_t>(P) + 1)) return rc;
        gatherSourcesKernel<<<gridFor(P, kWavesPerBlock), dim3(kBlock), 0, st>>>(P, ix.cluster_paths, table->source_off.ptr, table->source_id.ptr,
                                                                                pending.d_path_source_off.ptr, S, pending.d_source_id.ptr);
        clusterSourceOffKernel<<<gridFor(static_cast<uint64_t>(K) + 1), dim3(kBlock), 0, st>>>(K, ix.cluster_path_off, pending.d_path_source_off.ptr,
                                                                                              b->cluster_src_off.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 3;
        b->h_cluster_src_off.assign(static_cast<size_t>(K) + 1, 0);
        RPVG_HIP_CHECK(hipMemcpyAsync(b->h_cluster_src_off.data(), b->cluster_src_off.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint64_t),
                                      hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(queuePathSourceKernels(ctx, b, pending, st));
    }
    b->h_cluster_total.assign(K, 0.0);
    if (K) {
        RPVG_HIP_CHECK(d_totals.alloc(K));
        RPVG_HIP_CHECK(queueClusterTotals(st, K, b->cluster_row_off.ptr, d_row_count_u32, d_totals.ptr));
        RPVG_HIP_CHECK(hipMemcpyAsync(b->h_cluster_total.data(), d_totals.ptr, K * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    span.end();
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return finishPathSources(b, pending);
}

}  // namespace rpvg_hip_detail

extern "C" {

int rpvg_hip_path_table_upload(rpvg_hip_ctx * ctx, const rpvg_path_table * in, rpvg_hip_path_table ** table_out) {
    RPVG_REQUIRE(ctx && in && table_out, "rpvg_hip_path_table_upload: NULL argument");
    *table_out = nullptr;
    const uint32_t P = in->num_paths;
    RPVG_REQUIRE(P < 0x7fffffffu, "rpvg_hip_path_table_upload: %u paths exceed one table", P);
    RPVG_REQUIRE(P == 0 || (in->group_id && in->source_count && in->length && in->effective_length), "rpvg_hip_path_table_upload: NULL array");
    RPVG_REQUIRE((in->source_off == nullptr) == (in->source_id == nullptr) || (in->source_off && in->num_sources == 0),
                 "rpvg_hip_path_table_upload: source_off and source_id go together");
    const bool sources = in->source_off != nullptr;
    const uint64_t S = sources ? in->num_sources : 0;
    RPVG_REQUIRE(sources || in->num_sources == 0, "rpvg_hip_path_table_upload: %llu sources without source arrays",
                 static_cast<unsigned long long>(in->num_sources));
    RPVG_REQUIRE(P > 0 || S == 0, "rpvg_hip_path_table_upload: source ids without paths");
    std::unique_ptr<rpvg_hip_path_table> t(new (std::nothrow) rpvg_hip_path_table());
    if (!t) {
        setError("rpvg_hip_path_table_upload: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    t->num_paths = P;
    t->num_sources = S;
    t->has_sources = sources;
    t->has_names = in->name_id != nullptr;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<unsigned long long> d_bad;
    unsigned long long bad = kNoBad;
    SpanScope copies(ctx, FAM_H2D);
    RPVG_HIP_CHECK(t->group_id.upload(in->group_id, P, st));
    RPVG_HIP_CHECK(t->source_count.upload(in->source_count, P, st));
    RPVG_HIP_CHECK(t->length.upload(in->length, P, st));
    RPVG_HIP_CHECK(t->effective_length.upload(in->effective_length, P, st));
    if (t->has_names) RPVG_HIP_CHECK(t->name_id.upload(in->name_id, P, st));
    if (sources) {
        RPVG_HIP_CHECK(t->source_off.upload(in->source_off, static_cast<size_t>(P) + 1, st));
        RPVG_HIP_CHECK(t->source_id.upload(in->source_id, S, st));
        RPVG_HIP_CHECK(d_bad.upload(&kNoBad, 1, st));
    }
    copies.end();
    ctx->stats.h2d_bytes += static_cast<double>(P) * (20 + (t->has_names ? 4 : 0) + (sources ? 8 : 0)) + static_cast<double>(S) * 4;
    if (sources && P) {
        SpanScope check(ctx, FAM_BUILD);
        validateTableKernel<<<gridFor(P), dim3(kBlock), 0, st>>>(P, S, t->source_off.ptr, d_bad.ptr);
        check.end();
        ctx->stats.build_launches += 1;
        RPVG_HIP_CHECK(hipGetLastError());
        RPVG_HIP_CHECK(hipMemcpyAsync(&bad, d_bad.ptr, sizeof(bad), hipMemcpyDeviceToHost, st));
    }
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != kNoBad) {
        const Offender o = offenderOf(bad, kBadEnd);
        const unsigned long long path = o.index;
        if (o.why == kBadEnd) {
            setError("rpvg_hip_path_table_upload: path %llu: source_off ends at another value than num_sources = %llu", path,
                     static_cast<unsigned long long>(S));
        } else {
            setError("rpvg_hip_path_table_upload: path %llu: source_off is not a non-decreasing sequence of offsets into source_id", path);
        }
        return RPVG_HIP_ERR_INVALID;
    }
    *table_out = t.release();
    return RPVG_HIP_OK;
}

void rpvg_hip_path_table_free(rpvg_hip_ctx * ctx, rpvg_hip_path_table * table) {
    if (!table) return;
    waitAndDelete(ctx);
    delete table;
}

int rpvg_hip_batch_path_group_ids(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t * group_ids_out) {
    RPVG_REQUIRE(ctx && batch && (group_ids_out || batch->num_paths == 0), "rpvg_hip_batch_path_group_ids: NULL argument");
    RPVG_REQUIRE(batch->path_group_id.count == batch->num_paths, "rpvg_hip_batch_path_group_ids: the batch has no path side");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(batch->path_group_id.download(group_ids_out, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

void rpvg_hip_name_groups_limits(rpvg_name_groups_limits * limits_out) {
    if (!limits_out) return;
    limits_out->wave_paths = kWavePaths;
    limits_out->lds_paths = kLdsPaths;
}

int rpvg_hip_align_index_name_groups(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * index, const rpvg_hip_path_table * table,
                                     rpvg_hip_name_groups ** groups_out) {
    RPVG_REQUIRE(ctx && index && table && groups_out, "rpvg_hip_align_index_name_groups: NULL argument");
    *groups_out = nullptr;
    AlignIndexParts ix;
    RPVG_REQUIRE(alignIndexParts(index, ix), "rpvg_hip_align_index_name_groups: the index is not finished");
    const uint32_t K = ix.num_clusters, P = ix.num_paths;
    RPVG_REQUIRE(table->num_paths == P, "rpvg_hip_align_index_name_groups: the table has %u paths, the index %u", table->num_paths, P);
    RPVG_REQUIRE(table->has_names || P == 0, "rpvg_hip_align_index_name_groups: the table has no name_id");
    std::unique_ptr<rpvg_hip_name_groups> g(new (std::nothrow) rpvg_hip_name_groups());
    if (!g) {
        setError("rpvg_hip_align_index_name_groups: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    g->num_clusters = K;
    g->num_paths = P;
    g->h_cluster_group_off.assign(static_cast<size_t>(K) + 1, 0);
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(g->path_group.alloc(P));
    RPVG_HIP_CHECK(g->cluster_group_off.alloc(static_cast<size_t>(K) + 1));
    if (K == 0 || P == 0) {
        RPVG_HIP_CHECK(zeroAsync(g->cluster_group_off.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint64_t), st));
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        *groups_out = g.release();
        return RPVG_HIP_OK;
    }
    const dim3 block(kBlock);
    DeviceBuffer<uint32_t> group_count, mid_list, counters, position_cluster;
    RPVG_HIP_CHECK(group_count.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(mid_list.alloc(K));
    RPVG_HIP_CHECK(counters.alloc(2));
    RPVG_HIP_CHECK(position_cluster.alloc(P));
    SpanScope span(ctx, FAM_BUILD);
    RPVG_HIP_CHECK(zeroAsync(group_count.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint32_t), st));
    RPVG_HIP_CHECK(zeroAsync(counters.ptr, 2 * sizeof(uint32_t), st));
    GroupArgs a;
    a.num_clusters = K;
    a.num_paths = P;
    a.cluster_path_off = ix.cluster_path_off;
    a.cluster_paths = ix.cluster_paths;
    a.name_id = table->name_id.ptr;
    a.path_group = g->path_group.ptr;
    a.group_count = group_count.ptr;
    a.mid_list = mid_list.ptr;
    a.counters = counters.ptr;
    waveGroupsKernel<<<gridFor(K, kWavesPerBlock), block, 0, st>>>(a);
    ldsGroupsKernel<<<dim3(std::min<uint32_t>(K, kLdsGrid)), block, 0, st>>>(a);
    positionClusterKernel<<<gridFor(P), block, 0, st>>>(P, K, ix.cluster_path_off, position_cluster.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 3;
    uint32_t h_counters[2] = {0, 0};
    RPVG_HIP_CHECK(hipMemcpyAsync(h_counters, counters.ptr, sizeof(h_counters), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    if (h_counters[1]) {  // some cluster is beyond LDS: the global route
        DeviceBuffer<unsigned long long> key, key_sorted;
        DeviceBuffer<uint32_t> position, position_sorted, head, run_head, first_position, is_head, head_rank;
        RPVG_HIP_CHECK(key.alloc(P));
        RPVG_HIP_CHECK(key_sorted.alloc(P));
        RPVG_HIP_CHECK(position.alloc(P));
        RPVG_HIP_CHECK(position_sorted.alloc(P));
        RPVG_HIP_CHECK(head.alloc(P));
        RPVG_HIP_CHECK(run_head.alloc(P));
        RPVG_HIP_CHECK(first_position.alloc(P));
        RPVG_HIP_CHECK(is_head.alloc(static_cast<size_t>(P) + 1));
        RPVG_HIP_CHECK(head_rank.alloc(static_cast<size_t>(P) + 1));
        globalKeysKernel<<<gridFor(P), block, 0, st>>>(P, position_cluster.ptr, ix.cluster_paths, table->name_id.ptr, key.ptr, position.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = sortPairs(st, key.ptr, key_sorted.ptr, position.ptr, position_sorted.ptr, P, 32 + bitsFor(K))) return rc;
        runHeadKernel<unsigned long long><<<gridFor(P), block, 0, st>>>(P, key_sorted.ptr, head.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = inclusiveScan(st, head.ptr, run_head.ptr, MaxU32(), P)) return rc;
        firstPositionKernel<<<gridFor(P), block, 0, st>>>(P, position_sorted.ptr, run_head.ptr, first_position.ptr);
        headFlagKernel<<<gridFor(static_cast<uint64_t>(P) + 1), block, 0, st>>>(P, first_position.ptr, is_head.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = exclusiveSum(st, is_head.ptr, head_rank.ptr, static_cast<uint64_t>(P) + 1)) return rc;
        globalGroupsKernel<<<gridFor(P), block, 0, st>>>(a, position_cluster.ptr, first_position.ptr, head_rank.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 5;
    }
    if (const int rc = exclusiveSum(st, group_count.ptr, g->cluster_group_off.ptr, static_cast<uint64_t>(K) + 1)) return rc;
    RPVG_HIP_CHECK(hipMemcpyAsync(g->h_cluster_group_off.data(), g->cluster_group_off.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t G = g->h_cluster_group_off[K];
    if (G == 0 || G > P) {
        (void) hipDeviceSynchronize();
        setError("rpvg_hip_align_index_name_groups: %llu groups of %u paths", static_cast<unsigned long long>(G), P);
        return RPVG_HIP_ERR_RUNTIME;
    }
    g->num_groups = G;

    // the members of every group in ascending position, then one thread per group
    DeviceBuffer<uint32_t> gkey, gkey_sorted, position, member, member_off;
    DeviceBuffer<unsigned long long> d_bad;
    unsigned long long bad = kNoBad;
    RPVG_HIP_CHECK(gkey.alloc(P));
    RPVG_HIP_CHECK(gkey_sorted.alloc(P));
    RPVG_HIP_CHECK(position.alloc(P));
    RPVG_HIP_CHECK(member.alloc(P));
    RPVG_HIP_CHECK(member_off.alloc(G + 1));
    RPVG_HIP_CHECK(d_bad.upload(&kNoBad, 1, st));
    RPVG_HIP_CHECK(g->group_first_path.alloc(G));
    RPVG_HIP_CHECK(g->group_name_id.alloc(G));
    RPVG_HIP_CHECK(g->group_group_id.alloc(G));
    RPVG_HIP_CHECK(g->group_source_count.alloc(G));
    RPVG_HIP_CHECK(g->group_length.alloc(G));
    RPVG_HIP_CHECK(g->group_effective_length.alloc(G));
    groupKeyKernel<<<gridFor(P), block, 0, st>>>(P, position_cluster.ptr, g->cluster_group_off.ptr, g->path_group.ptr, gkey.ptr, position.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    if (const int rc = sortPairs(st, gkey.ptr, gkey_sorted.ptr, position.ptr, member.ptr, P, bitsFor(G))) return rc;
    groupStartKernel<<<gridFor(static_cast<uint64_t>(P) + 1), block, 0, st>>>(P, G, gkey_sorted.ptr, member_off.ptr);
    CollapseArgs c;
    c.num_groups = G;
    c.num_paths = P;
    c.member_off = member_off.ptr;
    c.member = member.ptr;
    c.cluster_paths = ix.cluster_paths;
    c.name_id = table->name_id.ptr;
    c.group_id = table->group_id.ptr;
    c.source_count = table->source_count.ptr;
    c.length = table->length.ptr;
    c.effective_length = table->effective_length.ptr;
    c.out_first_path = g->group_first_path.ptr;
    c.out_name_id = g->group_name_id.ptr;
    c.out_group_id = g->group_group_id.ptr;
    c.out_source_count = g->group_source_count.ptr;
    c.out_length = g->group_length.ptr;
    c.out_effective_length = g->group_effective_length.ptr;
    c.bad = d_bad.ptr;
    collapseGroupsKernel<<<gridFor(G), block, 0, st>>>(c);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 3;
    RPVG_HIP_CHECK(hipMemcpyAsync(&bad, d_bad.ptr, sizeof(bad), hipMemcpyDeviceToHost, st));
    span.end();
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != kNoBad) {
        const Offender o = offenderOf(bad, kBadLength);
        const uint64_t group = o.index;
        const uint32_t cluster = static_cast<uint32_t>(std::upper_bound(g->h_cluster_group_off.begin(), g->h_cluster_group_off.end(), group) -
                                                       g->h_cluster_group_off.begin()) - 1;
        static const char * const reasons[] = {"", "has a path with a source count of 0", "has a summed source count beyond 32 bits",
                                               "has a length beyond 32 bits"};
        setError("rpvg_hip_align_index_name_groups: group %llu of cluster %u %s", static_cast<unsigned long long>(group - g->h_cluster_group_off[cluster]),
                 cluster, reasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    *groups_out = g.release();
    return RPVG_HIP_OK;
}

int rpvg_hip_name_groups_view(rpvg_hip_ctx * ctx, rpvg_hip_name_groups * g, rpvg_name_groups_view * view) {
    RPVG_REQUIRE(ctx && g && view, "rpvg_hip_name_groups_view: NULL argument");
    if (!g->downloaded) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint64_t G = g->num_groups;
        int rc = downloadVector(st, g->path_group.ptr, g->num_paths, g->h_path_group);
        if (!rc) rc = downloadVector(st, g->group_first_path.ptr, G, g->h_group_first_path);
        if (!rc) rc = downloadVector(st, g->group_name_id.ptr, G, g->h_group_name_id);
        if (!rc) rc = downloadVector(st, g->group_group_id.ptr, G, g->h_group_group_id);
        if (!rc) rc = downloadVector(st, g->group_source_count.ptr, G, g->h_group_source_count);
        if (!rc) rc = downloadVector(st, g->group_length.ptr, G, g->h_group_length);
        if (!rc) rc = downloadVector(st, g->group_effective_length.ptr, G, g->h_group_effective_length);
        if (rc) return rc;
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        g->downloaded = true;
    }
    std::memset(view, 0, sizeof(*view));
    view->num_clusters = g->num_clusters;
    view->num_paths = g->num_paths;
    view->path_group = g->h_path_group.data();
    view->cluster_group_off = g->h_cluster_group_off.data();
    view->group_first_path = g->h_group_first_path.data();
    view->group_name_id = g->h_group_name_id.data();
    view->group_group_id = g->h_group_group_id.data();
    view->group_source_count = g->h_group_source_count.data();
    view->group_length = g->h_group_length.data();
    view->group_effective_length = g->h_group_effective_length.data();
    return RPVG_HIP_OK;
}

void rpvg_hip_name_groups_free(rpvg_hip_ctx * ctx, rpvg_hip_name_groups * groups) {
    if (!groups) return;
    waitAndDelete(ctx);
    delete groups;
}

}  // extern "C"

// rows_merge.hip — the sort and merge of a cluster's rows behind the per-read kernels of read_rows.hip.
//
// Takes over   the caller's sort + quickMergeIdentical of adjacent rows      src/main.cpp:953-973
//              (operator<, quickMergeIdentical                               src/read_path_probabilities.cpp:223-322)
//
// The schedule of the sort — which clusters sort in one workgroup, the tiles of the larger ones, the launches and their
// (k, j) — is planRowSort's (rows_plan.hpp); the kernels take the padded length and the pairing from the same header.

#include "common.hpp"
#include "device_algos.hpp"
#include "read_rows.hpp"
#include "rows_plan.hpp"

using namespace rpvg_hip_detail;
using namespace rpvg_rows_plan;

namespace {

constexpr double kDoublePrecision = 2.220446049250313e-16 * 100;  // Utils::double_precision, src/utils.hpp:81

__device__ __forceinline__ bool doubleCompareDev(const double a, const double b) {
    return (a == b) || (fabs(a - b) < fabs(fmin(a, b)) * kDoublePrecision);
}

// The caller of the reference sorts a cluster's rows with ReadPathProbabilities::operator< and merges each row into the
// head of the current run while quickMergeIdentical accepts it (src/main.cpp:953-973).  operator< compares doubles with
// Utils::doubleCompare (relative 2.2e-14) so that rows that agree up to rounding — reads whose alignments differ by
// a common score shift — become neighbours.  Such a comparison is not a strict weak order when values chain
// (a ~ b, b ~ c, a < c), which the sub-precision mass moved into the noise term does produce; merge-path sorts may
// then duplicate elements.  The rows of a cluster are therefore sorted with a bitonic NETWORK — data-oblivious
// compare-exchanges always yield a permutation — using the reference's comparison literally: one workgroup per
// cluster in LDS up to 2048 rows, global-memory stages for larger clusters.  Where the comparison is consistent the
// order equals the reference's (up to ties, which merge anyway); where it is not, the reference's own order is
// whatever std::sort happens to produce.

// ReadPathProbabilities::operator<, src/read_path_probabilities.cpp:283-322 (+ the row id as last key: deterministic)
struct RowLess {
    RowView v;
    __device__ bool operator()(const uint32_t lhs, const uint32_t rhs) const {
        const double nl = v.sc.row_noise[lhs], nr = v.sc.row_noise[rhs];
        if (!doubleCompareDev(nl, nr)) return nl < nr;
        const uint32_t bl = v.sc.row_ngroups[lhs], br = v.sc.row_ngroups[rhs];
        if (bl != br) return bl < br;
        const uint64_t el = v.align_path_off[v.read_align_off[lhs]], er = v.align_path_off[v.read_align_off[rhs]];
        for (uint32_t i = 0; i < bl; ++i) {
            const double pl = v.sc.grp_prob[el + i], pr = v.sc.grp_prob[er + i];
            if (!doubleCompareDev(pl, pr)) return pl < pr;
            const uint32_t sl = v.sc.grp_size[el + i], sr = v.sc.grp_size[er + i];
            if (sl != sr) return sl < sr;
            const uint32_t ml = v.sc.grp_moff[el + i], mr = v.sc.grp_moff[er + i];
            for (uint32_t j = 0; j < sl; ++j) {
                const uint32_t xl = v.sc.member[el + ml + j], xr = v.sc.member[er + mr + j];
                if (xl != xr) return xl < xr;
            }
        }
        const uint32_t tl = v.read_count[lhs], tr = v.read_count[rhs];
        if (tl != tr) return tl < tr;
        return lhs < rhs;
    }
};

// ReadPathProbabilities::quickMergeIdentical without the count update (src/read_path_probabilities.cpp:223-250)
__device__ bool mergeable(const RowView & v, const uint32_t a, const uint32_t b) {
    if (fabs(v.sc.row_noise[a] - v.sc.row_noise[b]) >= v.prob_precision) return false;
    const uint32_t nb = v.sc.row_ngroups[a];
    if (nb != v.sc.row_ngroups[b]) return false;
    const uint64_t ea = v.align_path_off[v.read_align_off[a]], eb = v.align_path_off[v.read_align_off[b]];
    for (uint32_t i = 0; i < nb; ++i) {
        if (fabs(v.sc.grp_prob[ea + i] - v.sc.grp_prob[eb + i]) >= v.prob_precision) return false;
        const uint32_t size = v.sc.grp_size[ea + i];
        if (size != v.sc.grp_size[eb + i]) return false;
        const uint32_t ma = v.sc.grp_moff[ea + i], mb = v.sc.grp_moff[eb + i];
        for (uint32_t j = 0; j < size; ++j) {
            if (v.sc.member[ea + ma + j] != v.sc.member[eb + mb + j]) return false;
        }
    }
    return true;
}

// The positions of a tile in LDS: row id plus the row's first sort keys (noise, number of groups, probability of the
// first group), which travel with the id.  RowLess reads its keys from global memory through a chain of dependent
// loads (row -> alignment offsets -> groups); most comparisons are decided by the first keys, which are the same
// values, so the outcome is RowLess's.
struct SortTile {
    uint32_t * id;
    uint32_t * ngroups;
    double * noise;
    double * prob0;

    __device__ void load(const RowLess & less, const uint32_t pos, const uint32_t row) {
        id[pos] = row;
        if (row == kNone) return;
        const uint32_t nb = less.v.sc.row_ngroups[row];
        noise[pos] = less.v.sc.row_noise[row];
        ngroups[pos] = nb;
        prob0[pos] = nb ? less.v.sc.grp_prob[less.v.align_path_off[less.v.read_align_off[row]]] : 0.0;
    }

    // is the row at position l before the row at position i?
    __device__ bool before(const RowLess & less, const uint32_t l, const uint32_t i) const {
        const double nl = noise[l], nr = noise[i];
        if (!doubleCompareDev(nl, nr)) return nl < nr;
        const uint32_t bl = ngroups[l], br = ngroups[i];
        if (bl != br) return bl < br;
        if (bl > 0) {
            const double pl = prob0[l], pr = prob0[i];
            if (!doubleCompareDev(pl, pr)) return pl < pr;
        }
        return less(id[l], id[i]);
    }

    __device__ void exchange(const RowLess & less, const uint32_t i, const uint32_t l) {
        const uint32_t a = id[i], b = id[l];
        if (b != kNone && (a == kNone || before(less, l, i))) {
            const double na = noise[i], pa = prob0[i];
            const uint32_t ga = ngroups[i];
            id[i] = b;
            noise[i] = noise[l];
            prob0[i] = prob0[l];
            ngroups[i] = ngroups[l];
            id[l] = a;
            noise[l] = na;
            prob0[l] = pa;
            ngroups[l] = ga;
        }
    }
};

#define RPVG_SORT_TILE_LDS(tile)                          \
    __shared__ uint32_t tile##_id[kSmallSort];            \
    __shared__ uint32_t tile##_ngroups[kSmallSort];       \
    __shared__ double tile##_noise[kSmallSort];           \
    __shared__ double tile##_prob0[kSmallSort];           \
    SortTile tile{tile##_id, tile##_ngroups, tile##_noise, tile##_prob0}

// one workgroup per cluster with at most kSmallSort rows; positions beyond the cluster's rows behave as +infinity
__global__ __launch_bounds__(256) void sortSmallClustersKernel(const uint32_t num_listed, const uint32_t * __restrict__ listed,
                                                               const uint64_t * __restrict__ cluster_read_off, const RowLess less,
                                                               uint32_t * __restrict__ sorted) {
    RPVG_SORT_TILE_LDS(tile);
    if (blockIdx.x >= num_listed) return;
    const uint32_t c = listed[blockIdx.x];
    const uint64_t r0 = cluster_read_off[c];
    const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
    const uint32_t L = sortPadded(n);
    for (uint32_t i = threadIdx.x; i < L; i += blockDim.x) tile.load(less, i, (i < n) ? static_cast<uint32_t>(r0 + i) : kNone);
    __syncthreads();
    for (uint32_t k = 2; k <= L; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (L >> 1); t += blockDim.x) {
                uint32_t i, l;
                bitonicPair(t, k, j, &i, &l);
                tile.exchange(less, i, l);
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) sorted[r0 + i] = tile.id[i];
}

// Clusters with more than kSmallSort rows: tiles of kSmallSort positions are sorted (first = true: all steps up to
// k = kSmallSort) or finished (first = false: the steps j = kSmallSort / 2 .. 1 of the merge of width k, which stay
// inside a tile) in LDS; only the steps that span tiles run through global memory (bitonicStepBigKernel).
__global__ __launch_bounds__(256) void sortTilesBigKernel(const uint32_t num_tiles, const uint32_t * __restrict__ tile_cluster,
                                                          const uint32_t * __restrict__ tile_index,
                                                          const uint64_t * __restrict__ cluster_read_off, const RowLess less,
                                                          const bool first, const uint32_t k_merge, uint32_t * __restrict__ sorted) {
    RPVG_SORT_TILE_LDS(tile);
    if (blockIdx.x >= num_tiles) return;
    const uint32_t c = tile_cluster[blockIdx.x];
    const uint64_t r0 = cluster_read_off[c];
    const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
    const uint32_t base = tile_index[blockIdx.x] * kSmallSort;
    if (base >= n) return;  // a tile of padding only
    if (!first && k_merge > sortPadded(n)) return;  // this cluster's network is complete
    for (uint32_t i = threadIdx.x; i < kSmallSort; i += blockDim.x) tile.load(less, i, (base + i < n) ? sorted[r0 + base + i] : kNone);
    __syncthreads();
    if (first) {
        for (uint32_t k = 2; k <= kSmallSort; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = threadIdx.x; t < (kSmallSort >> 1); t += blockDim.x) {
                    uint32_t i, l;
                    bitonicPair(t, k, j, &i, &l);
                    tile.exchange(less, i, l);
                }
                __syncthreads();
            }
        }
    } else {
        for (uint32_t j = kSmallSort >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (kSmallSort >> 1); t += blockDim.x) {
                uint32_t i, l;
                bitonicPair(t, k_merge, j, &i, &l);  // j < k_merge / 2: the plain (i, i + j) pairing
                tile.exchange(less, i, l);
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < kSmallSort; i += blockDim.x) {
        if (base + i < n) sorted[r0 + base + i] = tile.id[i];
    }
}

// one step (k, j) of the network for the clusters with more than kSmallSort rows: thread = (big cluster, pair)
__global__ void bitonicStepBigKernel(const uint32_t num_big, const uint32_t * __restrict__ big_cluster,
                                     const uint64_t * __restrict__ big_pair_off, const uint32_t * __restrict__ big_padded,
                                     const uint64_t * __restrict__ cluster_read_off, const RowLess less, const uint32_t k,
                                     const uint32_t j, uint32_t * __restrict__ sorted) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (g >= big_pair_off[num_big]) return;
    uint32_t lo = 0, hi = num_big - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (big_pair_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    if (k > big_padded[lo]) return;
    const uint32_t c = big_cluster[lo];
    const uint64_t r0 = cluster_read_off[c];
    const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
    uint32_t i, l;
    bitonicPair(static_cast<uint32_t>(g - big_pair_off[lo]), k, j, &i, &l);
    if (l >= n) return;  // the partner is +infinity: already in order
    const uint32_t a = sorted[r0 + i], b = sorted[r0 + l];
    if (less(b, a)) {
        sorted[r0 + i] = b;
        sorted[r0 + l] = a;
    }
}

// head[i] = 1 when sorted row i cannot be merged into its predecessor (first guess at the runs); head_pos[i] = i then.
__global__ void adjacentHeadsKernel(const uint64_t n, const RowView v, const uint32_t * __restrict__ sorted,
                                    uint32_t * __restrict__ head, uint32_t * __restrict__ head_pos) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    bool h = true;
    if (i > 0) {
        const uint32_t a = sorted[i - 1], b = sorted[i];
        h = v.read_cluster[a] != v.read_cluster[b] || !mergeable(v, a, b);
    }
    head[i] = h;
    head_pos[i] = h ? static_cast<uint32_t>(i) : 0;
}

// The reference merges into the HEAD of the run (src/main.cpp:958-968), not into the predecessor: a row that
// matched its predecessor but not the head starts a new run.  Flags the clusters where that happens.
__global__ void checkRunHeadsKernel(const uint64_t n, const RowView v, const uint32_t * __restrict__ sorted,
                                    const uint32_t * __restrict__ head, const uint32_t * __restrict__ run_head_pos,
                                    uint32_t * __restrict__ cluster_needs_walk, uint32_t * __restrict__ any) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n || head[i]) return;
    if (!mergeable(v, sorted[run_head_pos[i]], sorted[i])) {
        cluster_needs_walk[v.read_cluster[sorted[i]]] = 1;
        *any = 1;
    }
}

// Exact sequential replay of src/main.cpp:953-973 for the flagged clusters (one thread each; rare).
__global__ void walkClustersKernel(const uint32_t num_clusters, const uint64_t * __restrict__ cluster_read_off, const RowView v,
                                   const uint32_t * __restrict__ sorted, const uint32_t * __restrict__ cluster_needs_walk,
                                   uint32_t * __restrict__ head) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_clusters || !cluster_needs_walk[k]) return;
    const uint64_t r0 = cluster_read_off[k], r1 = cluster_read_off[k + 1];
    uint64_t cur = r0;
    for (uint64_t i = r0; i < r1; ++i) {
        if (i == r0) {
            head[i] = 1;
        } else if (mergeable(v, sorted[cur], sorted[i])) {
            head[i] = 0;
        } else {
            head[i] = 1;
            cur = i;
        }
    }
}

// run_incl[i] (inclusive sum of head flags) - 1 = merged row of sorted row i
__global__ void mergeRunsKernel(const uint64_t n, const RowView v, const uint32_t * __restrict__ sorted,
                                const uint32_t * __restrict__ head, const uint32_t * __restrict__ run_incl,
                                uint32_t * __restrict__ source, uint32_t * __restrict__ merged_count) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint32_t run = run_incl[i] - 1;
    const uint32_t r = sorted[i];
    atomicAdd(merged_count + run, v.read_count[r]);  // integer: order-free
    if (head[i]) source[run] = r;
}

__global__ void clusterRowOffKernel(const uint32_t num_clusters, const uint64_t num_reads, const uint64_t num_merged,
                                    const uint64_t * __restrict__ cluster_read_off, const uint32_t * __restrict__ run_incl,
                                    uint64_t * __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > num_clusters) return;
    const uint64_t r = cluster_read_off[k];
    out[k] = (r < num_reads) ? run_incl[r] - 1 : num_merged;
}

// ---- the host stage ---------------------------------------------------------------------------------------------------------

// One merge: what its stages share.  The lists of the sort live here because the kernels that read them are still queued when
// sortStage returns (the pool hands a freed block to the next allocation).
struct MergeState {
    hipStream_t st;
    const rpvg_hip_alignments * al;
    uint32_t K;
    uint64_t N;
    RowView view;
    DeviceBuffer<uint32_t> d_sorted, d_head, d_head_pos, d_run_head, d_walk, d_any, d_run_incl;
    DeviceBuffer<uint32_t> d_small, d_big, d_big_padded, d_tile_cluster, d_tile_index;
    DeviceBuffer<uint64_t> d_big_pair_off;
};

// sorts the rows of every cluster: queues the launches of the plan in its order
int sortStage(MergeState & s) {
    hipStream_t st = s.st;
    const RowLess less{s.view};
    const uint64_t * cluster_read_off = s.al->cluster_read_off.ptr;
    const RowSortPlan plan = planRowSort(s.al->h_cluster_read_off.data(), s.K);
    iotaKernel<<<dim3(plan.iota.grid), dim3(plan.iota.block), 0, st>>>(s.N, s.d_sorted.ptr);
    if (plan.sort_small.grid) {
        RPVG_HIP_CHECK(s.d_small.upload(plan.small_clusters.data(), plan.small_clusters.size(), st));
        sortSmallClustersKernel<<<dim3(plan.sort_small.grid), dim3(plan.sort_small.block), 0, st>>>(plan.sort_small.grid, s.d_small.ptr, cluster_read_off,
                                                                                                  less, s.d_sorted.ptr);
    }
    if (!plan.big_launches.empty()) {
        RPVG_HIP_CHECK(s.d_big.upload(plan.big_clusters.data(), plan.big_clusters.size(), st));
        RPVG_HIP_CHECK(s.d_big_padded.upload(plan.big_padded.data(), plan.big_padded.size(), st));
        RPVG_HIP_CHECK(s.d_big_pair_off.upload(plan.big_pair_off.data(), plan.big_pair_off.size(), st));
        RPVG_HIP_CHECK(s.d_tile_cluster.upload(plan.tile_cluster.data(), plan.tile_cluster.size(), st));
        RPVG_HIP_CHECK(s.d_tile_index.upload(plan.tile_index.data(), plan.tile_index.size(), st));
    }
    const uint32_t num_big = static_cast<uint32_t>(plan.big_clusters.size()), num_tiles = static_cast<uint32_t>(plan.tile_cluster.size());
    for (const SortLaunch & launch : plan.big_launches) {
        const dim3 grid(launch.shape.grid), block(launch.shape.block);
        if (launch.kind == SortStep::GlobalStep) {
            bitonicStepBigKernel<<<grid, block, 0, st>>>(num_big, s.d_big.ptr, s.d_big_pair_off.ptr, s.d_big_padded.ptr, cluster_read_off, less,
                                                         launch.k, launch.j, s.d_sorted.ptr);
        } else {
            sortTilesBigKernel<<<grid, block, 0, st>>>(num_tiles, s.d_tile_cluster.ptr, s.d_tile_index.ptr, cluster_read_off, less,
                                                       launch.kind == SortStep::TileSort, launch.k, s.d_sorted.ptr);
        }
    }
    RPVG_HIP_CHECK(hipGetLastError());
    return RPVG_HIP_OK;
}

// the runs of the sorted rows: head flags, corrected where a row matches its predecessor but not the head of its run, and
// their inclusive sum; *num_runs = the merged rows
int runsStage(MergeState & s, uint64_t * num_runs) {
    hipStream_t st = s.st;
    const uint64_t N = s.N;
    adjacentHeadsKernel<<<gridFor(N), dim3(256), 0, st>>>(N, s.view, s.d_sorted.ptr, s.d_head.ptr, s.d_head_pos.ptr);
    if (const int rc = inclusiveScan(st, s.d_head_pos.ptr, s.d_run_head.ptr, MaxU32(), N)) return rc;
    RPVG_HIP_CHECK(hipMemsetAsync(s.d_walk.ptr, 0, sizeof(uint32_t) * s.K, st));
    RPVG_HIP_CHECK(hipMemsetAsync(s.d_any.ptr, 0, sizeof(uint32_t), st));
    checkRunHeadsKernel<<<gridFor(N), dim3(256), 0, st>>>(N, s.view, s.d_sorted.ptr, s.d_head.ptr, s.d_run_head.ptr, s.d_walk.ptr, s.d_any.ptr);
    uint32_t any = 0;
    if (const int rc = fetchOne(st, s.d_any.ptr, &any)) return rc;
    if (any) {
        walkClustersKernel<<<gridFor(s.K, 64), dim3(64), 0, st>>>(s.K, s.al->cluster_read_off.ptr, s.view, s.d_sorted.ptr, s.d_walk.ptr, s.d_head.ptr);
    }
    if (const int rc = inclusiveSum(st, s.d_head.ptr, s.d_run_incl.ptr, N)) return rc;
    uint32_t last = 0;
    if (const int rc = fetchOne(st, s.d_run_incl.ptr + (N - 1), &last)) return rc;
    *num_runs = last;
    return RPVG_HIP_OK;
}

}  // namespace

int rpvg_hip_detail::mergeRows(rpvg_hip_ctx * ctx, const rpvg_hip_alignments * al, const RowsScratch & sc, const double prob_precision,
                               rpvg_hip_read_rows * out, DeviceBuffer<uint32_t> * d_source, uint64_t * num_out) {
    MergeState s;
    hipStream_t st = s.st = ctx->stream;
    s.al = al;
    const uint32_t K = s.K = al->num_clusters;
    const uint64_t N = s.N = al->num_reads;
    s.view = RowView{al->read_cluster.ptr, al->read_count.ptr, al->read_align_off.ptr, al->align_path_off.ptr, sc, prob_precision};
    RPVG_HIP_CHECK(s.d_sorted.alloc(N));
    RPVG_HIP_CHECK(s.d_head.alloc(N));
    RPVG_HIP_CHECK(s.d_head_pos.alloc(N));
    RPVG_HIP_CHECK(s.d_run_head.alloc(N));
    RPVG_HIP_CHECK(s.d_run_incl.alloc(N));
    RPVG_HIP_CHECK(s.d_walk.alloc(K));
    RPVG_HIP_CHECK(s.d_any.alloc(1));
    if (const int rc = sortStage(s)) return rc;
    if (const int rc = runsStage(s, num_out)) return rc;

    RPVG_HIP_CHECK(d_source->alloc(*num_out));
    RPVG_HIP_CHECK(out->row_count.alloc(*num_out));
    RPVG_HIP_CHECK(out->cluster_row_off.alloc(K + 1));
    RPVG_HIP_CHECK(hipMemsetAsync(out->row_count.ptr, 0, sizeof(uint32_t) * *num_out, st));
    mergeRunsKernel<<<gridFor(N), dim3(256), 0, st>>>(N, s.view, s.d_sorted.ptr, s.d_head.ptr, s.d_run_incl.ptr, d_source->ptr, out->row_count.ptr);
    clusterRowOffKernel<<<gridFor(K + 1), dim3(256), 0, st>>>(K, N, *num_out, al->cluster_read_off.ptr, s.d_run_incl.ptr, out->cluster_row_off.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    out->h_cluster_row_off.resize(K + 1);
    RPVG_HIP_CHECK(hipMemcpyAsync(out->h_cluster_row_off.data(), out->cluster_row_off.ptr, sizeof(uint64_t) * (K + 1), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the sort / scan buffers of `s` go out of scope here
    return RPVG_HIP_OK;
}

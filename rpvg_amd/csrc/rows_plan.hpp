// The host plan of the read rows (alignments.hip, read_rows.hip, rows_merge.hip): what an alignment batch is refused for and what
// its upload needs besides the copies, the sorting schedule of a merge — which clusters sort in one workgroup, which through
// tiles, and the launches of the tile and global steps in order — and the launch shapes of the row kernels and the pack.  A pure
// computation on the caller's host arrays and on sizes, plain C++17, no HIP types, no getenv, so that a CPU test reaches every
// decision and replays the schedule as a sorting network (tests/cpp/rows_plan_check.cpp).  The .hip files queue what the plan
// says.  The constants, readIsSmall(), sortPadded() and bitonicPair() are the kernels' too: host and device share one definition.
#ifndef RPVG_ROWS_PLAN_HPP
#define RPVG_ROWS_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rpvg_rows.h"

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_rows_plan {

constexpr uint32_t kSmallSort = 2048;  // rows one workgroup sorts in LDS: a cluster up to here, a tile of a larger one
constexpr int kGroupLanes = 16;        // lanes that share a read of at most that many (alignment, path) entries (readRowSmallKernel)
constexpr int kWavesPerBlock = 4;      // reads of a workgroup of readRowKernel: a wavefront each

// restated (alignments.hip asserts that they are rpvg_hip.h's)
constexpr int kStatusOk = 0, kStatusInvalid = -3;

// A read goes to the sixteen-lane kernel when its entries fit a group and nothing is collapsed (the name groups are
// readRowKernel's).  The index on the device (align_index.hip) splits with collapse = false and lists every read as large
// afterwards where it collapses.
RPVG_PLAN_FN bool readIsSmall(const uint64_t entries, const bool collapse) { return entries <= static_cast<uint64_t>(kGroupLanes) && !collapse; }

// Positions of the bitonic network of a cluster of n rows: a power of two, at least 2 up to kSmallSort rows (one workgroup), at
// least kSmallSort beyond (tiles); the positions from n on behave as +infinity.
RPVG_PLAN_FN uint32_t sortPadded(const uint32_t n) {
    uint32_t padded = n > kSmallSort ? kSmallSort : 2;
    while (padded < n) padded <<= 1;
    return padded;
}

// Pair t of step (k, j) of the all-ascending bitonic network: the first step of a merge of width k pairs i with its
// mirror image inside the block of k, the later steps pair i with i + j.
RPVG_PLAN_FN void bitonicPair(const uint32_t t, const uint32_t k, const uint32_t j, uint32_t * i, uint32_t * l) {
    if (j == (k >> 1)) {
        const uint32_t block = t / j, off = t % j;
        *i = block * k + off;
        *l = block * k + (k - 1 - off);
    } else {
        *i = 2 * j * (t / j) + (t % j);
        *l = *i + j;
    }
}

struct Launch {
    uint32_t grid = 0, block = 0;  // grid 0: not launched
};

inline uint32_t blocksFor(const uint64_t n, const uint32_t per_block) { return static_cast<uint32_t>((n + per_block - 1) / per_block); }

// ---- the upload of an alignment batch ------------------------------------------------------------------------------------

struct AlignmentBatchPlan {
    int status = kStatusOk;  // kStatusInvalid: refused, `message` says why and nothing else below holds
    std::string message;
    uint32_t K = 0;
    uint64_t N = 0, A = 0, E = 0, P = 0;
    bool collapse = false;
    std::vector<uint32_t> read_cluster;              // [N]
    std::vector<uint64_t> h_out_path_off;            // [K + 1] output columns of each cluster: paths, or name groups
    std::vector<uint32_t> small_reads, large_reads;  // readIsSmall() or not, ascending
    double h2d_bytes = 0;
};

namespace detail {
inline AlignmentBatchPlan refuse(const char * text) {
    AlignmentBatchPlan p;
    p.status = kStatusInvalid;
    p.message = text;
    return p;
}
template <typename Arg>
inline AlignmentBatchPlan refuse(const char * format, const Arg arg) {
    char text[512];
    std::snprintf(text, sizeof(text), format, arg);
    return refuse(text);
}
}  // namespace detail

// Everything rpvg_hip_alignments_upload decides before its first HIP call: the sizes, the O(input) validation of the invariants
// the kernels rely on, the cluster of every read, the output column offsets, the split of the reads between the two row kernels
// and the byte figure of the statistics.  Of several faults the one the loops meet first is reported.  An offset beyond its
// array's total (which a later descent must follow) counts as the descent, so that nothing outside the caller's arrays is read.
inline AlignmentBatchPlan planAlignmentBatch(const rpvg_alignment_batch & in) {
    typedef unsigned long long ull;
    const uint32_t K = in.num_clusters;
    if (!(in.cluster_read_off && in.cluster_path_off)) return detail::refuse("rpvg_hip_alignments_upload: NULL cluster offsets");
    const uint64_t N = in.cluster_read_off[K], P = in.cluster_path_off[K];
    if (!(N < 0xffffffffull)) return detail::refuse("rpvg_hip_alignments_upload: %llu reads exceed one call", static_cast<ull>(N));
    if (!(N == 0 || (in.read_count && in.read_min_mapq && in.read_noise_score && in.read_align_off))) {
        return detail::refuse("rpvg_hip_alignments_upload: NULL read arrays");
    }
    if (!(P == 0 || in.path_effective_length)) return detail::refuse("rpvg_hip_alignments_upload: NULL path_effective_length");
    const bool collapse = in.path_group != nullptr;
    if (!(!collapse || (in.cluster_group_off && in.path_source_count))) {
        return detail::refuse("rpvg_hip_alignments_upload: collapsing needs cluster_group_off and path_source_count");
    }
    const uint64_t A = N ? in.read_align_off[N] : 0;
    if (!(A == 0 || (in.align_score_sum && in.align_length && in.align_frag_length && in.align_path_off))) {
        return detail::refuse("rpvg_hip_alignments_upload: NULL alignment arrays");
    }
    const uint64_t E = A ? in.align_path_off[A] : 0;
    if (!(E == 0 || in.align_path_idx)) return detail::refuse("rpvg_hip_alignments_upload: NULL align_path_idx");
    if (!(E < 0xffffffffull)) return detail::refuse("rpvg_hip_alignments_upload: %llu path entries exceed one call", static_cast<ull>(E));

    AlignmentBatchPlan p;
    p.K = K;
    p.N = N;
    p.A = A;
    p.E = E;
    p.P = P;
    p.collapse = collapse;
    p.read_cluster.assign(N, 0);
    int bad = 0;
    for (uint32_t k = 0; k < K && !bad; ++k) {
        int why = 0;
        if (in.cluster_read_off[k] > in.cluster_read_off[k + 1] || in.cluster_path_off[k] > in.cluster_path_off[k + 1]) why = 1;
        if (in.cluster_read_off[k + 1] > N || in.cluster_path_off[k + 1] > P) why = 1;
        const uint64_t np = in.cluster_path_off[k + 1] - in.cluster_path_off[k];
        const uint64_t ng = collapse ? in.cluster_group_off[k + 1] - in.cluster_group_off[k] : 0;
        for (uint64_t q = in.cluster_path_off[k]; !why && collapse && q < in.cluster_path_off[k + 1]; ++q) {
            if (in.path_group[q] >= ng || in.path_source_count[q] == 0) why = 2;
        }
        for (uint64_t r = in.cluster_read_off[k]; !why && r < in.cluster_read_off[k + 1]; ++r) {
            p.read_cluster[r] = k;
            if (in.read_align_off[r] >= in.read_align_off[r + 1] || in.read_align_off[r + 1] > A) why = 3;
            if (in.read_noise_score[r] > 0) why = 4;
            for (uint64_t a = in.read_align_off[r]; !why && a < in.read_align_off[r + 1]; ++a) {
                if (in.align_path_off[a] >= in.align_path_off[a + 1] || in.align_path_off[a + 1] > E || in.align_length[a] == 0) why = 5;
                for (uint64_t e = in.align_path_off[a]; !why && e < in.align_path_off[a + 1]; ++e) {
                    if (in.align_path_idx[e] >= np || (e > in.align_path_off[a] && in.align_path_idx[e - 1] >= in.align_path_idx[e])) why = 6;
                }
            }
        }
        if (why) bad = why;
    }
    static const char * const reasons[] = {"", "descending cluster offsets", "a path group outside its cluster or a zero source count",
                                           "a read without alignments", "a read with a positive noise score",
                                           "an alignment without paths or with zero length",
                                           "path indices of an alignment must be ascending and inside the cluster"};
    if (bad) return detail::refuse("rpvg_hip_alignments_upload: %s", reasons[bad]);

    p.h_out_path_off.assign(static_cast<size_t>(K) + 1, 0);
    for (uint32_t k = 0; k < K; ++k) {
        p.h_out_path_off[k + 1] = p.h_out_path_off[k] + (collapse ? in.cluster_group_off[k + 1] - in.cluster_group_off[k]
                                                                  : in.cluster_path_off[k + 1] - in.cluster_path_off[k]);
    }
    for (uint64_t r = 0; r < N; ++r) {
        const uint64_t entries = in.align_path_off[in.read_align_off[r + 1]] - in.align_path_off[in.read_align_off[r]];
        (readIsSmall(entries, collapse) ? p.small_reads : p.large_reads).push_back(static_cast<uint32_t>(r));
    }
    p.h2d_bytes = static_cast<double>(N) * 25 + static_cast<double>(A) * 16 + static_cast<double>(E) * 4 + static_cast<double>(P) * 8;
    return p;
}

// ---- the sort of a merge ---------------------------------------------------------------------------------------------------
// The rows of every cluster are sorted with an all-ascending bitonic network over sortPadded() positions.  A cluster of 2 to
// kSmallSort rows takes one workgroup of sortSmallClustersKernel.  A larger one is cut into tiles of kSmallSort positions: one
// launch sorts every tile (all steps up to k = kSmallSort); then, for every merge width k up to the largest padded length of the
// call, the steps that span tiles (j >= kSmallSort) take one launch of bitonicStepBigKernel each over the pairs of all big
// clusters and one launch finishes the steps inside the tiles.  A cluster whose padded length is below k sits those launches
// out (the kernels' `k > padded` exits), and so does a tile of padding only.

enum class SortStep {
    TileSort,    // sortTilesBigKernel, first = true
    GlobalStep,  // bitonicStepBigKernel, step (k, j)
    TileFinish,  // sortTilesBigKernel, first = false, k_merge = k
};

struct SortLaunch {
    SortStep kind;
    uint32_t k, j;  // TileSort: 0, 0; TileFinish: k, 0
    Launch shape;
};

struct RowSortPlan {
    std::vector<uint32_t> small_clusters;             // 2 .. kSmallSort rows
    std::vector<uint32_t> big_clusters, big_padded;   // more: the cluster and its sortPadded()
    std::vector<uint64_t> big_pair_off;               // [big + 1] padded / 2 pairs each
    std::vector<uint32_t> tile_cluster, tile_index;   // padded / kSmallSort tiles of every big cluster, in order
    uint32_t max_padded = 0;
    Launch iota, sort_small;
    std::vector<SortLaunch> big_launches;             // in their order on the stream, behind iota and sort_small
};

inline RowSortPlan planRowSort(const uint64_t * cluster_read_off, const uint32_t K) {
    RowSortPlan p;
    p.big_pair_off.assign(1, 0);
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t n = cluster_read_off[k + 1] - cluster_read_off[k];
        if (n < 2) continue;
        if (n <= kSmallSort) {
            p.small_clusters.push_back(k);
        } else {
            const uint32_t padded = sortPadded(static_cast<uint32_t>(n));
            p.big_clusters.push_back(k);
            p.big_padded.push_back(padded);
            p.big_pair_off.push_back(p.big_pair_off.back() + padded / 2);
            p.max_padded = std::max(p.max_padded, padded);
            for (uint32_t t = 0; t < padded / kSmallSort; ++t) {
                p.tile_cluster.push_back(k);
                p.tile_index.push_back(t);
            }
        }
    }
    p.iota = Launch{blocksFor(K ? cluster_read_off[K] : 0, 256), 256};
    if (!p.small_clusters.empty()) p.sort_small = Launch{static_cast<uint32_t>(p.small_clusters.size()), 256};
    if (p.big_clusters.empty()) return p;
    const Launch tiles{static_cast<uint32_t>(p.tile_cluster.size()), 256}, pairs{blocksFor(p.big_pair_off.back(), 256), 256};
    p.big_launches.push_back(SortLaunch{SortStep::TileSort, 0, 0, tiles});
    for (uint32_t k = 2 * kSmallSort; k <= p.max_padded; k <<= 1) {
        for (uint32_t j = k >> 1; j >= kSmallSort; j >>= 1) p.big_launches.push_back(SortLaunch{SortStep::GlobalStep, k, j, pairs});
        p.big_launches.push_back(SortLaunch{SortStep::TileFinish, k, 0, tiles});
    }
    return p;
}

// ---- launch shapes of the row kernels and the pack ------------------------------------------------------------------------

struct RowKernelsPlan {
    Launch align_log_prob;  // alignLogProbKernel: a thread per alignment
    Launch small_reads;     // readRowSmallKernel over the small list: kGroupLanes lanes per read
    Launch large_reads;     // readRowKernel: a wavefront per read
    bool every_read = false;  // readRowKernel takes reads 0 .. N - 1 without a list (the small kernel switched off)
};

inline RowKernelsPlan planRowKernels(const uint64_t N, const uint64_t A, const uint64_t num_small, const uint64_t num_large, const bool small_kernel) {
    RowKernelsPlan p;
    p.align_log_prob = Launch{blocksFor(A, 256), 256};
    p.every_read = !small_kernel;
    if (p.every_read) {
        p.large_reads = Launch{blocksFor(N, kWavesPerBlock), 64 * kWavesPerBlock};
        return p;
    }
    if (num_small) p.small_reads = Launch{blocksFor(num_small * kGroupLanes, 256), 256};
    if (num_large) p.large_reads = Launch{blocksFor(num_large, kWavesPerBlock), 64 * kWavesPerBlock};
    return p;
}

struct PackPlan {
    Launch gather_sizes;  // gatherSizesKernel: a thread per output row
    Launch pack;          // packRowsKernel: kGroupLanes lanes per output row
};

// num_rows: all reads, or the runs a merge left
inline PackPlan planPack(const uint64_t num_rows) {
    return PackPlan{Launch{blocksFor(num_rows, 256), 256}, Launch{blocksFor(num_rows * kGroupLanes, 256), 256}};
}

}  // namespace rpvg_rows_plan

#endif

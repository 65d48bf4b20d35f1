// From the full enumeration of the haplotype sets to the merged estimates without a host round trip (gfx950): ploidy 1 and 3 .. 8.
//
// NestedPathAbundanceEstimator::inferAbundancesCollapsedGroups (src/path_abundance_estimator.cpp:428-471) with exact posteriors is
//   calculatePathGroupPosteriorsFull         src/path_estimator.cpp:332-377             (group_full.hip, queueGroupFullLaunch)
//   selectPathSubsetIndices                  src/path_abundance_estimator.cpp:569-606   <- fullRetainKernel + fullSelectKernel
//   inferPathSubsetAbundance, per subset     :625-671                                   (fullExpandKernel, then em_sparse.hip)
//   the posterior-weighted merge             :702-749                                   <- fullMergeKernel
// subset_em.hip does this for the diploid search, whose kept pairs are few; here a matrix has up to 2^31 sets, and the separate
// calls brought every posterior to the host to find the at most 1 / min_hap_prob that matter.  The posteriors of a launch stay on the
// device and are read once more:
//   fullRetainKernel    one pass over the posteriors of a launch: the (rank, posterior) of every set at or above min_hap_prob into
//                       the slots of its matrix (at most 1 024: posteriors sum to one) — a ballot and one integer atomic per
//                       wavefront and matrix claim the slots, in arrival order
//   fullSelectKernel    one workgroup per matrix: the slots sorted by rank in LDS (ranks are distinct: the arrival order is gone),
//                       members from ranks (unrankSet, subset_full_plan.hpp), every set's path list walked as a group_size-way merge
//                       of its columns' ascending lists (cursors in registers, never stored), identical lists merged by adding
//                       their posteriors in ascending rank (:595-596), weights over the sum of the kept posteriors (:598-605), the
//                       `weight < min_hap_prob` check (:627-630), subsets in lexicographic order of their lists
//   subsetOffsetsKernel, packResultsKernel   subset_pack.hpp: the diploid call's, unchanged
//   fullExpandKernel    subsetExpandKernel's job for group_size columns
//   fullMergeKernel     one workgroup per matrix: a record per (subset, transcript) keyed by the transcript's paths in list order
//                       (1 .. group_size of them, repeats kept) and the subset's rank; records sorted by a comparison on the whole
//                       tuple (eight paths do not fit the 64-bit key of the diploid merge), runs added up by one thread each in
//                       subset order with separately rounded products, quotients and sums (the host merge's, bit for bit)
// The host reads the header while the EM runs and copies one block behind it, as the diploid call does.

#include "common.hpp"
#include "subset_pack.hpp"

#include <cmath>
#include <memory>
#include <vector>

using namespace rpvg_hip_detail;

namespace {

using rpvg_subset_full::kMaxSlots;
constexpr uint32_t kNoPath = 0xffffffffu;
constexpr uint32_t kFullMergeLdsRecords = 1024;  // records of a matrix whose keys are sorted in LDS

// ---- retain ------------------------------------------------------------------------------------------------------------------
struct RetainArgs {
    uint32_t P;                      // problems of the launch = the matrices first_matrix .. first_matrix + P
    uint32_t first_matrix;
    const uint64_t * set_off;        // [P+1] of the launch
    const double * posterior;        // [set_off[P]]
    const uint64_t * slot_off;       // [M+1]
    double min_hap_prob;
    uint32_t * count;                // [M] zero-initialised: sets at or above the threshold (may pass the slots: overflow)
    unsigned long long * slot_rank;
    double * slot_posterior;
};

__global__ __launch_bounds__(256) void fullRetainKernel(const RetainArgs args) {
    const uint64_t total = args.set_off[args.P];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    // (every wavefront runs the same number of rounds: the ballots below are taken by whole wavefronts)
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * blockDim.x; base < total; base += stride) {
        const uint64_t e = base + threadIdx.x;
        double value = 0.0;
        bool take = false;
        if (e < total) {
            value = args.posterior[e];
            take = value >= args.min_hap_prob;
        }
        unsigned long long pending = __ballot(take);
        if (pending == 0) continue;
        uint32_t q = 0;
        if (take) {  // last q with set_off[q] <= e
            uint32_t lo = 0, hi = args.P - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (args.set_off[mid] <= e) lo = mid; else hi = mid - 1;
            }
            q = lo;
        }
        while (pending) {
            const int leader = __ffsll(static_cast<long long>(pending)) - 1;
            const uint32_t leader_q = __shfl(q, leader, 64);
            const bool mine = take && q == leader_q;
            const unsigned long long same = __ballot(mine);
            const uint32_t m = args.first_matrix + leader_q;
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(&args.count[m], static_cast<uint32_t>(__popcll(same)));
            first = __shfl(first, leader, 64);
            if (mine) {
                const uint64_t slot0 = args.slot_off[m], slots = args.slot_off[m + 1] - slot0;
                const uint64_t at = first + static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
                if (at < slots) {
                    args.slot_rank[slot0 + at] = e - args.set_off[q];
                    args.slot_posterior[slot0 + at] = value;
                }
            }
            pending &= ~same;
        }
    }
}

// ---- the path list of a set: a GS-way merge of ascending column lists, walked through cursors --------------------------------
// (Materialising the lists would take slots x group_size x the longest column per matrix; the cursors are 3 x GS registers, and a
// comparison of two lists holds two walks: 48 VGPRs at group size 8.)
template <int GS>
struct SetWalk {
    const uint32_t * paths;  // the column lists of the matrix, from its first entry
    uint32_t pos[GS], end[GS], head[GS];
    __device__ __forceinline__ SetWalk(const uint64_t * group_path_off, const uint32_t * group_path, const uint64_t col0, const uint32_t * members) {
        const uint64_t path0 = group_path_off[col0];
        paths = group_path + path0;
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            const uint64_t column = col0 + members[i];
            pos[i] = static_cast<uint32_t>(group_path_off[column] - path0);
            end[i] = static_cast<uint32_t>(group_path_off[column + 1] - path0);
            head[i] = pos[i] < end[i] ? paths[pos[i]] : kNoPath;
        }
    }
    // the next path in ascending order (a path once per column that lists it); kNoPath behind the last
    __device__ __forceinline__ uint32_t next() {
        uint32_t best = head[0];
#pragma unroll
        for (int i = 1; i < GS; ++i) best = min(best, head[i]);
        if (best == kNoPath) return kNoPath;
        bool advanced = false;
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            if (!advanced && head[i] == best) {
                advanced = true;
                ++pos[i];
                head[i] = pos[i] < end[i] ? paths[pos[i]] : kNoPath;
            }
        }
        return best;
    }
};

// lexicographic comparison of two walks (std::vector's operator<: a list sorts before its extensions): -1, 0, 1
template <int GS>
__device__ __forceinline__ int compareWalks(SetWalk<GS> x, SetWalk<GS> y) {
    for (;;) {
        const uint32_t px = x.next(), py = y.next();
        if (px != py) {
            if (px == kNoPath) return -1;
            if (py == kNoPath) return 1;
            return px < py ? -1 : 1;
        }
        if (px == kNoPath) return 0;
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------------
struct FullSelectArgs {
    uint32_t num_matrices;
    const uint32_t * count;           // [M] fullRetainKernel's
    const uint64_t * slot_off;        // [M+1]
    unsigned long long * slot_rank;   // in: arrival order; out: ascending
    double * slot_posterior;
    uint32_t * slot_member;           // [slots x GS] members of the retained sets
    const uint64_t * group_off;       // [M+1]
    const uint64_t * group_path_off;
    const uint32_t * group_path;
    const uint32_t * cluster;         // [M]
    const uint64_t * cluster_row_off;
    const uint64_t * row_ent_off;
    double min_hap_prob;
    uint32_t segment_rows;
    uint32_t * retained;              // [M] retained sets of the matrix (0 on overflow)
    uint32_t * sub_set;               // per subset slot: the retained set (index within the matrix) that leads it
    double * slot_weight;
    uint32_t * slot_length;
    uint32_t * slot_columns;
    MatrixTotals * totals;
    SubsetHeader * header;
};

template <int GS>
__global__ __launch_bounds__(256) void fullSelectKernel(const FullSelectArgs args) {
    constexpr int BLOCK = 256;
    constexpr uint32_t CAP = kMaxSlots;
    __shared__ unsigned long long s_rank[CAP];  // ranks, then the hashes of the lists
    __shared__ double s_post[CAP];
    __shared__ double s_weight[CAP];
    __shared__ uint32_t s_length[CAP];
    __shared__ uint32_t s_leader[CAP];
    __shared__ uint32_t s_order[CAP];
    __shared__ double sum_posterior;
    __shared__ unsigned long long red[3];
    __shared__ uint32_t n_retained;
    const uint32_t m = blockIdx.x, tid = threadIdx.x;
    if (m >= args.num_matrices) return;
    const uint64_t slot0 = args.slot_off[m], slots = args.slot_off[m + 1] - slot0;
    const uint32_t cnt = args.count[m];
    MatrixTotals * out_totals = args.totals + m;
    if (cnt > slots || cnt > CAP) {  // (posteriors sum to one and min_hap_prob >= 1 / 1024: not reached with finite inputs)
        if (tid == 0) {
            atomicAdd(&args.header->select_overflow, 1ull);
            *out_totals = MatrixTotals{0, 0, 0, 0, 0, 0};
            args.retained[m] = 0;
        }
        return;
    }
    const uint64_t col0 = args.group_off[m];
    const uint32_t G = static_cast<uint32_t>(args.group_off[m + 1] - col0);
    // ascending by rank (ranks are distinct: what the atomics' arrival order left is gone)
    uint32_t padded = 1;
    while (padded < cnt) padded <<= 1;
    for (uint32_t i = tid; i < padded; i += BLOCK) {
        s_rank[i] = i < cnt ? args.slot_rank[slot0 + i] : ~0ull;
        s_post[i] = i < cnt ? args.slot_posterior[slot0 + i] : 0.0;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= padded; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < padded; i += BLOCK) {
                const uint32_t partner = i ^ stride;
                if (partner > i) {
                    const unsigned long long a = s_rank[i], b = s_rank[partner];
                    if ((a > b) == ((i & size) == 0)) {
                        s_rank[i] = b;
                        s_rank[partner] = a;
                        const double pa = s_post[i];
                        s_post[i] = s_post[partner];
                        s_post[partner] = pa;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t s = tid; s < cnt; s += BLOCK) {
        args.slot_rank[slot0 + s] = s_rank[s];
        args.slot_posterior[slot0 + s] = s_post[s];
        uint32_t members[GS];
        rpvg_subset_full::unrankSet(G, GS, s_rank[s], members);
#pragma unroll
        for (int i = 0; i < GS; ++i) args.slot_member[(slot0 + s) * GS + i] = members[i];
    }
    if (tid == 0) {
        double sum = 0;  // in ascending rank, as the reference adds it up (:598)
        for (uint32_t s = 0; s < cnt; ++s) sum += s_post[s];
        sum_posterior = sum;
        red[0] = red[1] = red[2] = 0;
        n_retained = 0;
        args.retained[m] = cnt;
    }
    __threadfence_block();
    __syncthreads();
    auto walk = [&](const uint32_t s) { return SetWalk<GS>(args.group_path_off, args.group_path, col0, args.slot_member + (slot0 + s) * GS); };
    // every set's path list: length and a hash (FNV-1a over the merged walk)
    unsigned long long * s_hash = s_rank;
    for (uint32_t s = tid; s < cnt; s += BLOCK) {
        SetWalk<GS> list = walk(s);
        unsigned long long h = 1469598103934665603ull;
        uint32_t n = 0;
        for (uint32_t path = list.next(); path != kNoPath; path = list.next()) {
            h = (h ^ path) * 1099511628211ull;
            ++n;
        }
        s_hash[s] = h;
        s_length[s] = n;
    }
    __syncthreads();
    // identical lists: the first of them (lowest rank) leads (:595, emplace finds the existing key)
    for (uint32_t s = tid; s < cnt; s += BLOCK) {
        uint32_t lead = s;
        for (uint32_t t = 0; t < s; ++t) {
            if (s_hash[t] == s_hash[s] && s_length[t] == s_length[s] && compareWalks<GS>(walk(t), walk(s)) == 0) {
                lead = t;
                break;
            }
        }
        s_leader[s] = lead;
    }
    __syncthreads();
    // mass of a subset: the posteriors of its sets added in ascending rank (:596), over the sum of all kept (:602-605); subsets
    // below the threshold are skipped (:627-630)
    for (uint32_t s = tid; s < cnt; s += BLOCK) {
        double w = 0;
        if (s_leader[s] == s) {
            for (uint32_t t = s; t < cnt; ++t) {
                if (s_leader[t] == s) w += s_post[t];
            }
            w /= sum_posterior;
            if (w >= args.min_hap_prob) s_order[atomicAdd(&n_retained, 1u)] = s;
        }
        s_weight[s] = w;
    }
    __syncthreads();
    // ... in lexicographic order of their lists (distinct lists: the order of the atomic above does not survive the sort)
    const uint32_t n_ret = n_retained;
    uint32_t padded_ret = 1;
    while (padded_ret < n_ret) padded_ret <<= 1;
    for (uint32_t i = n_ret + tid; i < padded_ret; i += BLOCK) s_order[i] = 0xffffffffu;
    __syncthreads();
    auto before = [&](const uint32_t x, const uint32_t y) {
        if (x == 0xffffffffu) return false;
        if (y == 0xffffffffu) return true;
        return compareWalks<GS>(walk(x), walk(y)) < 0;
    };
    for (uint32_t size = 2; size <= padded_ret; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < padded_ret; i += BLOCK) {
                const uint32_t partner = i ^ stride;
                if (partner > i) {
                    const bool ascending = (i & size) == 0;
                    const uint32_t x = s_order[i], y = s_order[partner];
                    if (before(y, x) == ascending) {
                        s_order[i] = y;
                        s_order[partner] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    unsigned long long my_subsets = 0, my_length = 0, my_columns = 0;
    for (uint32_t rank = tid; rank < n_ret; rank += BLOCK) {
        const uint32_t s = s_order[rank];
        uint32_t distinct = 0, previous = kNoPath;
        SetWalk<GS> list = walk(s);
        for (uint32_t path = list.next(); path != kNoPath; path = list.next()) {
            distinct += (path != previous) ? 1u : 0u;
            previous = path;
        }
        args.sub_set[slot0 + rank] = s;
        args.slot_weight[slot0 + rank] = s_weight[s];
        args.slot_length[slot0 + rank] = s_length[s];
        args.slot_columns[slot0 + rank] = distinct;
        my_subsets += 1;
        my_length += s_length[s];
        my_columns += distinct;
    }
    if (my_subsets) {
        atomicAdd(&red[0], my_subsets);
        atomicAdd(&red[1], my_length);
        atomicAdd(&red[2], my_columns);
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t k = args.cluster[m];
        const uint64_t r0 = args.cluster_row_off[k], r1 = args.cluster_row_off[k + 1];
        const unsigned long long rows = r1 - r0, entries = args.row_ent_off[r1] - args.row_ent_off[r0];
        *out_totals = MatrixTotals{red[0], red[1], red[2], red[0] * rows, red[0] * entries, red[0] * ((rows + args.segment_rows - 1) / args.segment_rows)};
    }
}

// ---- where the retained sets of every matrix go in the packed block: one workgroup, prefix sums over the matrices -------------
struct RetainedOffsetsArgs {
    uint32_t num_matrices, group_size;
    const uint32_t * retained;       // [M]
    unsigned long long * retained_off;  // [M+1]
    SubsetHeader * header;
};

__global__ __launch_bounds__(1024) void fullRetainedOffsetsKernel(const RetainedOffsetsArgs args) {
    __shared__ unsigned long long sums[1024];
    const uint32_t M = args.num_matrices;
    const uint32_t per = (M + 1023) / 1024;
    const uint32_t lo = min(M, threadIdx.x * per), hi = min(M, lo + per);
    unsigned long long mine = 0;
    for (uint32_t m = lo; m < hi; ++m) mine += args.retained[m];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t step = 1; step < 1024; step <<= 1) {
        unsigned long long add = 0;
        if (threadIdx.x >= step) add = sums[threadIdx.x - step];
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = sums[threadIdx.x] - mine;
    for (uint32_t m = lo; m < hi; ++m) {
        args.retained_off[m] = run;
        run += args.retained[m];
    }
    if (threadIdx.x == 1023) {
        args.retained_off[M] = sums[1023];
        args.header->retained = sums[1023];
        args.header->group_size = args.group_size;
    }
}

// ---- expand ------------------------------------------------------------------------------------------------------------------
struct FullExpandArgs {
    uint32_t num_matrices;
    const SubsetHeader * header;
    const MatrixTotals * totals;
    const MatrixTotals * bases;
    const uint64_t * slot_off;
    const uint32_t * sub_set;
    const uint32_t * slot_member;
    const double * slot_weight;
    const uint32_t * slot_length;
    const uint32_t * slot_columns;
    const uint64_t * group_off;
    const uint64_t * group_path_off;
    const uint32_t * group_path;
    const uint32_t * cluster;
    const uint64_t * cluster_row_off;
    const uint64_t * row_ent_off;
    // per subset
    uint32_t * sub_cluster;
    double * sub_weight;
    uint64_t * path_off;
    uint32_t * path;
    uint64_t * col_off;
    uint32_t * col_path;
    uint64_t * row_base;
    uint64_t * ent_base;
    uint64_t * seg_first;
    uint32_t * item_problem;
    uint32_t segment_rows;
    uint64_t * subset_off;   // [M+1]
};

template <int GS>
__global__ __launch_bounds__(256) void fullExpandKernel(const FullExpandArgs args) {
    constexpr int BLOCK = 256;
    __shared__ uint32_t scratch[BLOCK / 64];
    const uint32_t m = blockIdx.x;
    if (m >= args.num_matrices) return;
    const MatrixTotals base = args.bases[m];
    if (threadIdx.x == 0) {
        args.subset_off[m] = args.header->overflow ? 0 : base.subsets;
        if (m + 1 == args.num_matrices) args.subset_off[m + 1] = args.header->overflow ? 0 : args.header->subsets;
    }
    if (args.header->overflow) return;
    const uint32_t n = static_cast<uint32_t>(args.totals[m].subsets);
    const uint64_t slot0 = args.slot_off[m];
    const uint64_t col0 = args.group_off[m];
    const uint32_t k = args.cluster[m];
    const uint64_t r0 = args.cluster_row_off[k], r1 = args.cluster_row_off[k + 1];
    const uint64_t rows = r1 - r0, entries = args.row_ent_off[r1] - args.row_ent_off[r0];
    uint64_t length_run = base.list_length, columns_run = base.columns;
    for (uint32_t c = 0; c < n; c += BLOCK) {
        const uint32_t r = c + threadIdx.x;
        const uint32_t len = r < n ? args.slot_length[slot0 + r] : 0u, cols = r < n ? args.slot_columns[slot0 + r] : 0u;
        uint32_t len_total, cols_total;
        const uint32_t len_before = blockExclusiveScan<BLOCK>(len, len_total, scratch);
        const uint32_t cols_before = blockExclusiveScan<BLOCK>(cols, cols_total, scratch);
        if (r < n) {
            const uint64_t s = base.subsets + r;
            const uint64_t p0 = length_run + len_before, c0 = columns_run + cols_before;
            args.sub_cluster[s] = k;
            args.sub_weight[s] = args.slot_weight[slot0 + r];
            args.path_off[s] = p0;
            args.col_off[s] = c0;
            args.row_base[s] = base.rows + static_cast<uint64_t>(r) * rows;
            args.ent_base[s] = base.entries + static_cast<uint64_t>(r) * entries;
            const uint64_t segments = (rows + args.segment_rows - 1) / args.segment_rows, item0 = base.segments + static_cast<uint64_t>(r) * segments;
            args.seg_first[s] = item0;
            for (uint64_t item = item0; item < item0 + segments; ++item) args.item_problem[item] = static_cast<uint32_t>(s);
            SetWalk<GS> list(args.group_path_off, args.group_path, col0, args.slot_member + (slot0 + args.sub_set[slot0 + r]) * GS);
            uint32_t previous = kNoPath;
            uint64_t pw = p0, cw = c0;
            for (uint32_t path = list.next(); path != kNoPath; path = list.next()) {
                args.path[pw++] = path;
                // collapsed_path_subset (:637-656): the distinct paths, ascending = the columns of the subset's EM problem
                if (path != previous) args.col_path[cw++] = path;
                previous = path;
            }
        }
        length_run += len_total;
        columns_run += cols_total;
    }
}

// ---- the posterior-weighted merge for sets of up to GS paths (src/path_abundance_estimator.cpp:702-749) ------------------------
// Every position of every subset's list looks for the other paths of its transcript in the list; the first of them emits a record
//   key = [ path + 1 of the transcript's 1st .. GS-th path in list order, 0 where there is none | rank of the subset in the matrix ]
// (zero padding puts a list before its extensions, as std::vector's operator< does).  An index array is sorted by a comparison on
// the GS + 1 words (bitonic network; keys in LDS up to kFullMergeLdsRecords list entries per matrix, in device memory beyond), which
// puts the sets in the reference's order and the records of a set in subset order.  One thread per set adds its records up.
struct FullMergeArgs {
    const SubsetHeader * header;
    uint32_t num_matrices;
    const uint64_t * subset_off;
    const double * weight;
    const uint64_t * path_off;
    const uint32_t * path;
    const uint64_t * col_off;
    const uint32_t * col_path;
    const double * abundances;
    const double * noise;
    const double * total;
    const uint32_t * cluster;
    const uint64_t * cluster_path_off;
    const uint32_t * path_group_id;
    uint32_t * sort_key;     // [2 x capacity of the lists x (GS + 1)] of the matrices beyond LDS
    uint32_t * sort_pos;     // [2 x capacity of the lists]
    double * rec_abund;      // [capacity of the lists x GS]
    uint32_t * merge_bad;    // zero-initialised: set when a transcript has more than GS paths in one subset
    unsigned char * packed;
};

template <int GS>
__global__ __launch_bounds__(256) void fullMergeKernel(const FullMergeArgs args) {
    constexpr int BLOCK = 256;
    constexpr int W = GS + 1;
    __shared__ uint32_t s_key[kFullMergeLdsRecords * W];
    __shared__ uint32_t s_pos[kFullMergeLdsRecords];
    __shared__ uint32_t s_scan[BLOCK / 64];
    const SubsetHeader h = *args.header;
    if (h.overflow) return;
    const uint32_t m = blockIdx.x, tid = threadIdx.x;
    const uint64_t M = args.num_matrices;
    if (m >= M) return;
    const PackedLayout lay = packedLayout(M, h.subsets, h.list_length, h.columns, GS, h.retained);
    uint32_t * set_count = reinterpret_cast<uint32_t *>(args.packed + lay.set_count);
    double * cluster_noise = reinterpret_cast<double *>(args.packed + lay.cluster_noise);
    uint32_t * set_size = reinterpret_cast<uint32_t *>(args.packed + lay.set_size);
    uint32_t * set_member = reinterpret_cast<uint32_t *>(args.packed + lay.set_member);
    double * set_posterior = reinterpret_cast<double *>(args.packed + lay.set_posterior);
    double * set_abund = reinterpret_cast<double *>(args.packed + lay.set_abund);
    const uint64_t s0 = args.subset_off[m];
    const uint32_t n = static_cast<uint32_t>(args.subset_off[m + 1] - s0);
    if (n == 0) {  // (no set reached min_hap_prob: all reads are noise, :749 — the caller fills that in)
        if (tid == 0) {
            set_count[m] = 0;
            cluster_noise[m] = 0.0;
        }
        return;
    }
    const uint64_t base = args.path_off[s0];
    const uint32_t Lm = static_cast<uint32_t>(args.path_off[s0 + n] - base);
    const uint32_t * gid = args.path_group_id + args.cluster_path_off[args.cluster[m]];
    if (tid == BLOCK - 1) {  // the noise count, formed as subsetMergeKernel forms it (:712,749)
        double noise = 0.0, sum_hap_prob = 0.0;
        for (uint32_t r = 0; r < n; ++r) {
            const double w = args.weight[s0 + r];
            sum_hap_prob = addRounded(sum_hap_prob, w);
            noise = addRounded(noise, mulRounded(args.noise[s0 + r], w));
        }
        cluster_noise[m] = addRounded(noise, mulRounded(addRounded(1.0, -sum_hap_prob), args.total[s0]));
    }
    uint32_t P2 = 2;
    while (P2 < Lm) P2 <<= 1;
    uint32_t * keys = s_key;
    uint32_t * order = s_pos;
    if (P2 > kFullMergeLdsRecords) {
        keys = args.sort_key + 2 * base * W;
        order = args.sort_pos + 2 * base;
    }
    for (uint32_t pos = tid; pos < P2; pos += BLOCK) {
        uint32_t key[W];
#pragma unroll
        for (int i = 0; i < W; ++i) key[i] = 0;
        key[0] = kNoPath;  // no record
        if (pos < Lm) {
            uint32_t lo = 0, hi = n - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (args.path_off[s0 + mid] - base <= pos) lo = mid; else hi = mid - 1;
            }
            const uint32_t r = lo;
            const uint32_t l0 = static_cast<uint32_t>(args.path_off[s0 + r] - base), L = static_cast<uint32_t>(args.path_off[s0 + r + 1] - base) - l0;
            const uint32_t * list = args.path + base + l0;
            const uint32_t j = pos - l0;
            const uint32_t g = gid[list[j]];
            uint32_t members = 0, first = 0;
            for (uint32_t t = 0; t < L; ++t) {
                if (gid[list[t]] == g) {
                    if (members == 0) first = t;
                    ++members;
                }
            }
            if (members > GS) *args.merge_bad = 1;
            if (first == j && members <= GS) {
                const double w = args.weight[s0 + r];
                const uint64_t c0 = args.col_off[s0 + r];
                const uint32_t C = static_cast<uint32_t>(args.col_off[s0 + r + 1] - c0);
                const uint32_t * cols = args.col_path + c0;
                uint32_t filled = 0;
                for (uint32_t t = first; t < L && filled < members; ++t) {
                    const uint32_t p = list[t];
                    if (gid[p] != g) continue;
                    uint32_t a = 0, b = C;  // the path's column of the subset's EM problem
                    while (a < b) {
                        const uint32_t mid = (a + b) >> 1;
                        if (cols[mid] < p) a = mid + 1; else b = mid;
                    }
                    uint32_t multiplicity = 0;  // std::count over the subset's list (:737)
                    for (uint32_t u = 0; u < L; ++u) multiplicity += (list[u] == p) ? 1u : 0u;
                    args.rec_abund[(base + pos) * GS + filled] = mulRounded(args.abundances[c0 + a], w) / static_cast<double>(multiplicity);
#pragma unroll
                    for (int i = 0; i < GS; ++i) {
                        if (static_cast<uint32_t>(i) == filled) key[i] = p + 1;
                    }
                    ++filled;
                }
                for (uint32_t i = filled; i < GS; ++i) args.rec_abund[(base + pos) * GS + i] = 0.0;
                key[GS] = r;
            }
        }
#pragma unroll
        for (int i = 0; i < W; ++i) keys[static_cast<uint64_t>(pos) * W + i] = key[i];
        order[pos] = pos;
    }
    __threadfence_block();
    __syncthreads();
    auto after = [&](const uint32_t x, const uint32_t y) {  // record x sorts behind record y (distinct records never tie)
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const uint32_t a = keys[static_cast<uint64_t>(x) * W + i], b = keys[static_cast<uint64_t>(y) * W + i];
            if (a != b) return a > b;
        }
        return x > y;  // (two positions without a record)
    };
    for (uint32_t k2 = 2; k2 <= P2; k2 <<= 1) {
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = tid; i < P2; i += BLOCK) {
                const uint32_t x = i ^ j2;
                if (x > i) {
                    const uint32_t oa = order[i], ob = order[x];
                    if (after(oa, ob) == ((i & k2) == 0)) {
                        order[i] = ob;
                        order[x] = oa;
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    auto sameSet = [&](const uint32_t x, const uint32_t y) {
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            if (keys[static_cast<uint64_t>(x) * W + i] != keys[static_cast<uint64_t>(y) * W + i]) return false;
        }
        return true;
    };
    uint32_t Q = 0;
    for (uint32_t c0 = 0; c0 < Lm; c0 += BLOCK) {
        const uint32_t i = c0 + tid;
        const uint32_t rec = i < Lm ? order[i] : 0u;
        const bool is_record = i < Lm && keys[static_cast<uint64_t>(rec) * W] != kNoPath;
        const bool start = is_record && (i == 0 || !sameSet(order[i - 1], rec));
        uint32_t total;
        const uint32_t before = blockExclusiveSum<BLOCK>(start ? 1u : 0u, total, s_scan);
        if (start) {
            double posterior = 0.0, sums[GS];
#pragma unroll
            for (int a = 0; a < GS; ++a) sums[a] = 0.0;
            for (uint32_t e = i; e < Lm; ++e) {
                const uint32_t other = order[e];
                if (keys[static_cast<uint64_t>(other) * W] == kNoPath || !sameSet(other, rec)) break;
                const uint32_t r = keys[static_cast<uint64_t>(other) * W + GS];
                posterior = addRounded(posterior, args.weight[s0 + r]);
#pragma unroll
                for (int a = 0; a < GS; ++a) sums[a] = addRounded(sums[a], args.rec_abund[(base + other) * GS + a]);
            }
            const uint64_t q = base + Q + before;
            uint32_t size = 0;
#pragma unroll
            for (int a = 0; a < GS; ++a) {
                const uint32_t word = keys[static_cast<uint64_t>(rec) * W + a];
                size += word ? 1u : 0u;
                set_member[q * GS + a] = word ? word - 1 : kNoPath;
                set_abund[q * GS + a] = word ? sums[a] : 0.0;
            }
            set_size[q] = size;
            set_posterior[q] = posterior;
        }
        Q += total;
    }
    if (tid == 0) set_count[m] = Q;
}

// ---- the retained sets into the packed block ---------------------------------------------------------------------------------
struct RetainedPackArgs {
    const SubsetHeader * header;
    uint32_t num_matrices;
    const uint64_t * slot_off;
    const uint32_t * retained;
    const unsigned long long * retained_off;
    const unsigned long long * slot_rank;
    const double * slot_posterior;
    unsigned char * packed;
};

__global__ __launch_bounds__(256) void fullRetainedPackKernel(const RetainedPackArgs args) {
    const SubsetHeader h = *args.header;
    if (h.overflow) return;
    const uint64_t M = args.num_matrices;
    const uint32_t m = blockIdx.x;
    if (m >= M) return;
    const PackedLayout lay = packedLayout(M, h.subsets, h.list_length, h.columns, h.group_size, h.retained);
    unsigned long long * off = reinterpret_cast<unsigned long long *>(args.packed + lay.retained_off);
    unsigned long long * rank = reinterpret_cast<unsigned long long *>(args.packed + lay.retained_rank);
    double * posterior = reinterpret_cast<double *>(args.packed + lay.retained_posterior);
    const unsigned long long to = args.retained_off[m];
    const uint64_t from = args.slot_off[m];
    if (threadIdx.x == 0) {
        off[m] = to;
        if (m + 1 == M) off[M] = args.retained_off[M];
    }
    for (uint32_t i = threadIdx.x; i < args.retained[m]; i += blockDim.x) {
        rank[to + i] = args.slot_rank[from + i];
        posterior[to + i] = args.slot_posterior[from + i];
    }
}

// what the enumeration left on the device: the retained sets of every matrix in its slots (arrival order until the first select)
struct RetainedSets {
    uint32_t M = 0;
    std::vector<uint64_t> slot_off;
    uint64_t slots = 0, total_sets = 0;
    DeviceBuffer<uint64_t> d_slot_off;
    DeviceBuffer<uint32_t> d_count;
    DeviceBuffer<unsigned long long> d_slot_rank;
    DeviceBuffer<double> d_slot_posterior;
};

}  // namespace

// fullMergeKernel for a caller in another file (subset_independent.hip: its units are clusters, and group size 2 is among them)
void rpvg_hip_detail::queueFullMerge(const uint32_t group_size, const FullMergeLaunch & launch, hipStream_t st) {
    FullMergeArgs ma;
    ma.header = static_cast<const SubsetHeader *>(launch.header);
    ma.num_matrices = launch.num_units;
    ma.subset_off = launch.subset_off;
    ma.weight = launch.weight;
    ma.path_off = launch.path_off;
    ma.path = launch.path;
    ma.col_off = launch.col_off;
    ma.col_path = launch.col_path;
    ma.abundances = launch.abundances;
    ma.noise = launch.noise;
    ma.total = launch.total;
    ma.cluster = launch.cluster;
    ma.cluster_path_off = launch.cluster_path_off;
    ma.path_group_id = launch.path_group_id;
    ma.sort_key = launch.sort_key;
    ma.sort_pos = launch.sort_pos;
    ma.rec_abund = launch.rec_abund;
    ma.merge_bad = launch.merge_bad;
    ma.packed = launch.packed;
    const dim3 grid(launch.num_units), block(256);
    switch (group_size) {
        case 1: fullMergeKernel<1><<<grid, block, 0, st>>>(ma); break;
        case 2: fullMergeKernel<2><<<grid, block, 0, st>>>(ma); break;
        case 3: fullMergeKernel<3><<<grid, block, 0, st>>>(ma); break;
        case 4: fullMergeKernel<4><<<grid, block, 0, st>>>(ma); break;
        case 5: fullMergeKernel<5><<<grid, block, 0, st>>>(ma); break;
        case 6: fullMergeKernel<6><<<grid, block, 0, st>>>(ma); break;
        case 7: fullMergeKernel<7><<<grid, block, 0, st>>>(ma); break;
        default: fullMergeKernel<8><<<grid, block, 0, st>>>(ma); break;
    }
}

// The first stage: every launch of the enumeration, each followed by the pass that keeps its sets at or above the threshold.  The
// posterior buffer is one launch's and is reused; nothing proportional to the number of sets leaves the device.
static int queueEnumerationAndRetain(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, const uint32_t group_size, const double * log_freq,
                                     const double min_hap_prob, const std::vector<uint64_t> & sets, RetainedSets & kept,
                                     std::vector<std::unique_ptr<GroupFullLaunch> > & launches, DeviceBuffer<double> & d_posterior) {
    hipStream_t st = ctx->stream;
    const uint32_t M = groups->num_matrices;
    kept.M = M;
    kept.slot_off.assign(M + 1, 0);
    for (uint32_t m = 0; m < M; ++m) {
        kept.slot_off[m + 1] = kept.slot_off[m] + rpvg_subset_full::slotsOf(sets[m]);
        kept.total_sets += sets[m];
    }
    kept.slots = kept.slot_off[M];
    RPVG_HIP_CHECK(kept.d_slot_off.upload(kept.slot_off.data(), M + 1, st));
    RPVG_HIP_CHECK(kept.d_count.alloc(M));
    RPVG_HIP_CHECK(zeroAsync(kept.d_count.ptr, static_cast<size_t>(M) * 4, st));
    RPVG_HIP_CHECK(kept.d_slot_rank.alloc(kept.slots));
    RPVG_HIP_CHECK(kept.d_slot_posterior.alloc(kept.slots));
    // the launches, cut as rpvg_hip_group_full_posteriors cuts them; the posterior buffer holds the largest
    std::vector<uint32_t> matrix(M);
    for (uint32_t m = 0; m < M; ++m) matrix[m] = m;
    uint64_t largest = 0;
    for (uint32_t first = 0; first < M;) {
        const uint32_t end = rpvg_subset_full::chunkEnd(sets.data(), first, M);
        uint64_t launch_sets = 0;
        for (uint32_t q = first; q < end; ++q) launch_sets += sets[q];
        largest = std::max(largest, launch_sets);
        first = end;
    }
    RPVG_HIP_CHECK(d_posterior.alloc(largest));
    RPVG_HIP_CHECK(groups->waitCollapse(st));
    uint64_t lf_first = 0;
    for (uint32_t first = 0; first < M;) {
        const uint32_t end = rpvg_subset_full::chunkEnd(sets.data(), first, M);
        launches.emplace_back(new GroupFullLaunch());
        GroupFullLaunch & work = *launches.back();
        const int rc = queueGroupFullLaunch(ctx, groups, matrix.data() + first, end - first, sets.data() + first, group_size, log_freq + lf_first, work, d_posterior.ptr);
        if (rc != RPVG_HIP_OK) return rc;
        if (work.launch_sets) {
            RetainArgs ra;
            ra.P = end - first;
            ra.first_matrix = first;
            ra.set_off = work.d_set_off.ptr;
            ra.posterior = d_posterior.ptr;
            ra.slot_off = kept.d_slot_off.ptr;
            ra.min_hap_prob = min_hap_prob;
            ra.count = kept.d_count.ptr;
            ra.slot_rank = kept.d_slot_rank.ptr;
            ra.slot_posterior = kept.d_slot_posterior.ptr;
            const uint64_t blocks = std::min<uint64_t>((work.launch_sets + 255) / 256, 1u << 16);
            const int span = ctx->spanBegin(FAM_LOGLIK);
            fullRetainKernel<<<dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st>>>(ra);
            ctx->spanEnd(span);
            ctx->stats.loglik_launches += 1;
            RPVG_HIP_CHECK(hipGetLastError());
        }
        lf_first += work.lf_count;
        first = end;
    }
    return RPVG_HIP_OK;
}

// One attempt at everything behind the retained sets, with the capacities the context's hints give.  *did_not_fit: the reserved
// capacity was too small — the hints now hold what this very call needs and a second attempt fits.
static int nestedFullAttempt(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups, const uint32_t group_size,
                             const double min_hap_prob, const uint32_t max_em_its, const double max_rel_em_conv, const double collapse_precision,
                             RetainedSets & kept, const uint32_t max_paths, rpvg_hip_subset_em ** result_out, bool * did_not_fit) {
    *did_not_fit = false;
    const uint32_t M = groups->num_matrices;
    const uint32_t GS = group_size;
    hipStream_t st = ctx->stream;
    std::unique_ptr<rpvg_hip_subset_em> res(new (std::nothrow) rpvg_hip_subset_em());
    if (!res) {
        setError("rpvg_hip_nested_full_subset_em: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    res->num_matrices = M;
    uint64_t lane_rows = 0, lane_entries = 0, lane_paths = 0, max_cluster_work = 0;
    for (uint32_t m = 0; m < M; ++m) {
        const uint32_t k = groups->h_cluster[m];
        lane_rows += batch->h_cluster_row_off[k + 1] - batch->h_cluster_row_off[k];
        lane_entries += batch->h_cluster_ent_off[k + 1] - batch->h_cluster_ent_off[k];
        lane_paths += groups->h_num_paths[m];
        max_cluster_work = std::max<uint64_t>(max_cluster_work, (batch->h_cluster_row_off[k + 1] - batch->h_cluster_row_off[k]) +
                                                                    (batch->h_cluster_ent_off[k + 1] - batch->h_cluster_ent_off[k]));
    }
    const uint64_t slots = kept.slots;
    // Capacities: what the last call of this kind on the context needed, with headroom; a first call plans with eight subsets' worth
    // of every cluster.  A call that does not fit reports what it needed and is tried once more with exactly that.
    SubsetEmHints & hints = ctx->subset_full_hints;
    auto planned = [](const double per_unit, const unsigned long long units, const double headroom) {
        return static_cast<unsigned long long>(std::ceil(per_unit * headroom * static_cast<double>(units)));
    };
    unsigned long long cap_subsets = std::min<unsigned long long>(slots, hints.subsets_per_matrix > 0 ? planned(hints.subsets_per_matrix, M, 1.25) + 256 : std::max<unsigned long long>(8ull * M, 16384));
    unsigned long long cap_length = std::max<unsigned long long>(planned(hints.list_per_path, lane_paths, 2.0), std::max<unsigned long long>(4ull * GS * lane_paths, 1u << 18));
    unsigned long long cap_rows = hints.rows_per_row > 0 ? planned(hints.rows_per_row, lane_rows, 1.25) + 65536 : 8 * lane_rows;
    unsigned long long cap_entries = hints.entries_per_entry > 0 ? planned(hints.entries_per_entry, lane_entries, 1.25) + 65536 : 8 * lane_entries;
    if (hints.retry) {
        cap_subsets = std::min<unsigned long long>(slots, std::max(cap_subsets, hints.retry_subsets + 64));
        cap_length = std::max(cap_length, hints.retry_list_length + 64);
        cap_rows = std::max(cap_rows, hints.retry_rows + 64);
        cap_entries = std::max(cap_entries, hints.retry_entries + 64);
        hints.retry = false;
    }
    cap_subsets = std::max<unsigned long long>(cap_subsets, 1);
    const unsigned long long cap_columns = cap_length;
    const unsigned long long cap_items = cap_rows / emFillSegmentRows() + cap_subsets;

    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    // the header, the merge's flag word and a zero word behind it, and the EM work queues: one zeroed block
    const size_t header_room = 256;
    static_assert(sizeof(SubsetHeader) <= 192, "the merge's flag word sits behind the header");
    DeviceBuffer<unsigned char> d_zero;
    ok(d_zero.alloc(header_room + emQueuesBytes()));
    if (e == hipSuccess) ok(zeroAsync(d_zero.ptr, header_room + emQueuesBytes(), st));
    SubsetHeader * header = reinterpret_cast<SubsetHeader *>(d_zero.ptr);
    uint32_t * d_merge_bad = reinterpret_cast<uint32_t *>(d_zero.ptr + 192);
    const unsigned long long * d_zero_word = reinterpret_cast<const unsigned long long *>(d_zero.ptr + 200);
    DeviceBuffer<uint32_t> d_slot_member, d_retained, d_sub_set, d_slot_length, d_slot_columns;
    DeviceBuffer<double> d_slot_weight;
    DeviceBuffer<unsigned long long> d_retained_off;
    DeviceBuffer<unsigned char> d_totals, d_bases, d_packed;
    ok(d_slot_member.alloc(slots * GS));
    ok(d_retained.alloc(M));
    ok(d_retained_off.alloc(M + 1));
    ok(d_sub_set.alloc(slots));
    ok(d_slot_length.alloc(slots));
    ok(d_slot_columns.alloc(slots));
    ok(d_slot_weight.alloc(slots));
    ok(d_totals.alloc(sizeof(MatrixTotals) * M));
    ok(d_bases.alloc(sizeof(MatrixTotals) * M));
    DeviceBuffer<uint32_t> d_sub_cluster, d_path, d_col_path, d_iters, d_kept_rows, d_kept_entries, d_item_problem;
    DeviceBuffer<double> d_sub_weight, d_abund, d_noise, d_total;
    DeviceBuffer<uint64_t> d_path_off, d_col_off, d_row_base, d_ent_base, d_subset_off, d_seg_first;
    ok(d_sub_cluster.alloc(cap_subsets));
    ok(d_sub_weight.alloc(cap_subsets));
    ok(d_path_off.alloc(cap_subsets + 1));
    ok(d_col_off.alloc(cap_subsets + 1));
    ok(d_row_base.alloc(cap_subsets));
    ok(d_ent_base.alloc(cap_subsets));
    ok(d_subset_off.alloc(M + 1));
    ok(d_seg_first.alloc(cap_subsets + 1));
    ok(d_item_problem.alloc(cap_items));
    ok(d_path.alloc(cap_length));
    ok(d_col_path.alloc(cap_columns));
    ok(d_abund.alloc(cap_columns));
    ok(d_noise.alloc(cap_subsets));
    ok(d_total.alloc(cap_subsets));
    ok(d_iters.alloc(cap_subsets));
    ok(d_kept_rows.alloc(cap_subsets));
    ok(d_kept_entries.alloc(cap_subsets));
    ok(d_packed.alloc(packedLayout(M, cap_subsets, cap_length, cap_columns, GS, slots).bytes));
    DeviceBuffer<uint32_t> d_merge_key, d_merge_pos;
    DeviceBuffer<double> d_merge_abund;
    ok(d_merge_key.alloc((2 * cap_length + 2) * (GS + 1)));
    ok(d_merge_pos.alloc(2 * cap_length + 2));
    ok(d_merge_abund.alloc(cap_length * GS));
    void * pinned_header = nullptr;
    if (e == hipSuccess && pinnedAlloc(&pinned_header, sizeof(SubsetHeader)) != hipSuccess) e = hipErrorOutOfMemory;
    hipEvent_t header_here = nullptr;
    if (e == hipSuccess) ok(hipEventCreateWithFlags(&header_here, hipEventDisableTiming));
    if (e != hipSuccess) {
        setError("rpvg_hip_nested_full_subset_em: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        if (pinned_header) pinnedFree(pinned_header);
        if (header_here) (void) hipEventDestroy(header_here);
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    MatrixTotals * totals = reinterpret_cast<MatrixTotals *>(d_totals.ptr);
    MatrixTotals * bases = reinterpret_cast<MatrixTotals *>(d_bases.ptr);

#define RPVG_FULL_DISPATCH(KERNEL, GRID, ARGS)                                              \
    switch (GS) {                                                                           \
        case 1: KERNEL<1><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        case 3: KERNEL<3><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        case 4: KERNEL<4><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        case 5: KERNEL<5><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        case 6: KERNEL<6><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        case 7: KERNEL<7><<<GRID, dim3(256), 0, st>>>(ARGS); break;                         \
        default: KERNEL<8><<<GRID, dim3(256), 0, st>>>(ARGS); break;                        \
    }

    int span = ctx->spanBegin(FAM_BUILD);
    FullSelectArgs sa;
    sa.num_matrices = M;
    sa.count = kept.d_count.ptr;
    sa.slot_off = kept.d_slot_off.ptr;
    sa.slot_rank = kept.d_slot_rank.ptr;
    sa.slot_posterior = kept.d_slot_posterior.ptr;
    sa.slot_member = d_slot_member.ptr;
    sa.group_off = groups->d_group_off;
    sa.group_path_off = groups->d_group_path_off;
    sa.group_path = groups->d_group_path;
    sa.cluster = groups->d_cluster;
    sa.cluster_row_off = batch->cluster_row_off.ptr;
    sa.row_ent_off = batch->row_ent_off.ptr;
    sa.min_hap_prob = min_hap_prob;
    sa.segment_rows = emFillSegmentRows();
    sa.retained = d_retained.ptr;
    sa.sub_set = d_sub_set.ptr;
    sa.slot_weight = d_slot_weight.ptr;
    sa.slot_length = d_slot_length.ptr;
    sa.slot_columns = d_slot_columns.ptr;
    sa.totals = totals;
    sa.header = header;
    RPVG_FULL_DISPATCH(fullSelectKernel, dim3(M), sa);
    RetainedOffsetsArgs ro;
    ro.num_matrices = M;
    ro.group_size = GS;
    ro.retained = d_retained.ptr;
    ro.retained_off = d_retained_off.ptr;
    ro.header = header;
    fullRetainedOffsetsKernel<<<dim3(1), dim3(1024), 0, st>>>(ro);
    const bool check_build = !groups->build_checked && groups->build_error_flag.ptr;
    OffsetsArgs oa;
    oa.pair_count = d_retained.ptr;  // (the header's kept_pairs: the retained sets)
    oa.log_evals = d_zero_word;
    oa.build_error = check_build ? groups->build_error_flag.ptr : nullptr;
    oa.num_matrices = M;
    oa.totals = totals;
    oa.bases = bases;
    oa.header = header;
    oa.cap_subsets = cap_subsets;
    oa.cap_length = cap_length;
    oa.cap_columns = cap_columns;
    oa.cap_rows = cap_rows;
    oa.cap_entries = cap_entries;
    oa.cap_items = cap_items;
    oa.seg_first = d_seg_first.ptr;
    oa.path_off = d_path_off.ptr;
    oa.col_off = d_col_off.ptr;
    subsetOffsetsKernel<<<dim3(1), dim3(1024), 0, st>>>(oa);
    // the header reaches the host while the rest runs
    SubsetHeader * h_header = static_cast<SubsetHeader *>(pinned_header);
    ok(hipMemcpyAsync(h_header, header, sizeof(SubsetHeader), hipMemcpyDeviceToHost, st));
    ok(hipEventRecord(header_here, st));
    FullExpandArgs ea;
    ea.num_matrices = M;
    ea.header = header;
    ea.totals = totals;
    ea.bases = bases;
    ea.slot_off = kept.d_slot_off.ptr;
    ea.sub_set = d_sub_set.ptr;
    ea.slot_member = d_slot_member.ptr;
    ea.slot_weight = d_slot_weight.ptr;
    ea.slot_length = d_slot_length.ptr;
    ea.slot_columns = d_slot_columns.ptr;
    ea.group_off = groups->d_group_off;
    ea.group_path_off = groups->d_group_path_off;
    ea.group_path = groups->d_group_path;
    ea.cluster = groups->d_cluster;
    ea.cluster_row_off = batch->cluster_row_off.ptr;
    ea.row_ent_off = batch->row_ent_off.ptr;
    ea.sub_cluster = d_sub_cluster.ptr;
    ea.sub_weight = d_sub_weight.ptr;
    ea.path_off = d_path_off.ptr;
    ea.path = d_path.ptr;
    ea.col_off = d_col_off.ptr;
    ea.col_path = d_col_path.ptr;
    ea.row_base = d_row_base.ptr;
    ea.ent_base = d_ent_base.ptr;
    ea.seg_first = d_seg_first.ptr;
    ea.item_problem = d_item_problem.ptr;
    ea.segment_rows = emFillSegmentRows();
    ea.subset_off = d_subset_off.ptr;
    RPVG_FULL_DISPATCH(fullExpandKernel, dim3(M), ea);
    ok(hipGetLastError());
    ctx->spanEnd(span);
    ctx->stats.build_launches += 4;

    EmProblemList list;
    list.P_bound = static_cast<uint32_t>(std::min<unsigned long long>(cap_subsets, 0xfffffffeull));
    list.d_num_problems = &header->num_problems;
    list.d_cluster = d_sub_cluster.ptr;
    list.d_col_off = d_col_off.ptr;
    list.d_col_path = d_col_path.ptr;
    list.d_row_base = d_row_base.ptr;
    list.d_ent_base = d_ent_base.ptr;
    list.rows_capacity = cap_rows;
    list.entries_capacity = cap_entries;
    list.d_seg_first = d_seg_first.ptr;
    list.d_item_problem = d_item_problem.ptr;
    list.items_bound = static_cast<uint32_t>(std::min<unsigned long long>(cap_items, 0xfffffffeull));
    list.d_num_items = &header->num_items;
    list.max_cols = max_paths + 1;
    list.max_cluster_paths = max_paths;
    list.max_cluster_work = max_cluster_work;
    list.wide_capacity = 0;
    EmOutputs out{d_abund.ptr, d_noise.ptr, d_iters.ptr, d_kept_rows.ptr, d_kept_entries.ptr, d_total.ptr};
    EmSolveWork work;
    work.zeroed_queues = d_zero.ptr + header_room;
    if (e == hipSuccess) {
        const int rc = queueEmSolve(ctx, batch, list, max_em_its, max_rel_em_conv, out, work, collapse_precision);
        if (rc != RPVG_HIP_OK) {
            (void) hipStreamSynchronize(st);
            (void) hipEventDestroy(header_here);
            pinnedFree(pinned_header);
            return rc;
        }
    }
    if (e == hipSuccess) {
        FullMergeArgs ma;
        ma.header = header;
        ma.num_matrices = M;
        ma.subset_off = d_subset_off.ptr;
        ma.weight = d_sub_weight.ptr;
        ma.path_off = d_path_off.ptr;
        ma.path = d_path.ptr;
        ma.col_off = d_col_off.ptr;
        ma.col_path = d_col_path.ptr;
        ma.abundances = d_abund.ptr;
        ma.noise = d_noise.ptr;
        ma.total = d_total.ptr;
        ma.cluster = groups->d_cluster;
        ma.cluster_path_off = batch->cluster_path_off.ptr;
        ma.path_group_id = batch->path_group_id.ptr;
        ma.sort_key = d_merge_key.ptr;
        ma.sort_pos = d_merge_pos.ptr;
        ma.rec_abund = d_merge_abund.ptr;
        ma.merge_bad = d_merge_bad;
        ma.packed = d_packed.ptr;
        const int merge_span = ctx->spanBegin(FAM_BUILD);
        RPVG_FULL_DISPATCH(fullMergeKernel, dim3(M), ma);
        RetainedPackArgs rp;
        rp.header = header;
        rp.num_matrices = M;
        rp.slot_off = kept.d_slot_off.ptr;
        rp.retained = d_retained.ptr;
        rp.retained_off = d_retained_off.ptr;
        rp.slot_rank = kept.d_slot_rank.ptr;
        rp.slot_posterior = kept.d_slot_posterior.ptr;
        rp.packed = d_packed.ptr;
        fullRetainedPackKernel<<<dim3(M), dim3(256), 0, st>>>(rp);
        ctx->spanEnd(merge_span);
        ctx->stats.build_launches += 2;
    }
#undef RPVG_FULL_DISPATCH
    PackArgs pa;
    pa.merge_bad = d_merge_bad;
    pa.header = header;
    pa.num_matrices = M;
    pa.subset_off = d_subset_off.ptr;
    pa.weight = d_sub_weight.ptr;
    pa.path_off = d_path_off.ptr;
    pa.col_off = d_col_off.ptr;
    pa.abundances = d_abund.ptr;
    pa.noise = d_noise.ptr;
    pa.total = d_total.ptr;
    pa.path = d_path.ptr;
    pa.col_path = d_col_path.ptr;
    pa.iterations = d_iters.ptr;
    pa.kept_rows = d_kept_rows.ptr;
    pa.kept_entries = d_kept_entries.ptr;
    pa.packed = d_packed.ptr;
    packResultsKernel<<<dim3(256), dim3(256), 0, st>>>(pa);
    ok(hipGetLastError());

    if (e == hipSuccess) ok(waitEvent(header_here));
    (void) hipEventDestroy(header_here);
    if (e != hipSuccess) {
        setError("rpvg_hip_nested_full_subset_em: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        pinnedFree(pinned_header);
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    const SubsetHeader got = *h_header;
    pinnedFree(pinned_header);
    {
        auto fold = [](double & held, const unsigned long long needed, const unsigned long long units) {
            held = std::max(0.9 * held, static_cast<double>(needed) / static_cast<double>(std::max<unsigned long long>(units, 1)));
        };
        fold(hints.subsets_per_matrix, got.subsets, M);
        fold(hints.list_per_path, got.list_length, lane_paths);
        fold(hints.rows_per_row, got.rows, lane_rows);
        fold(hints.entries_per_entry, got.entries, lane_entries);
    }
    if (got.build_bad) {
        (void) hipStreamSynchronize(st);
        setError(got.build_bad == 2 ? "rpvg_hip_groups_build: a group lists a path twice" : "rpvg_hip_groups_build: a group refers to a path outside its cluster");
        return RPVG_HIP_ERR_INVALID;
    }
    groups->build_checked = true;
    if (got.overflow) {
        (void) hipStreamSynchronize(st);  // (the kernels behind the header saw zero problems)
        setError("rpvg_hip_nested_full_subset_em: not taken (%llu subsets, %llu list entries, %llu rows, %llu entries, %llu matrices with more sets at "
                 "or above min_hap_prob than slots: over the reserved capacity)", got.subsets, got.list_length, got.rows, got.entries, got.select_overflow);
        if (!got.select_overflow) {
            hints.retry = true;
            hints.retry_subsets = got.subsets;
            hints.retry_list_length = std::max(got.list_length, got.columns);
            hints.retry_rows = got.rows;
            hints.retry_entries = got.entries;
            *did_not_fit = true;
        }
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    // exactly what there is: one block, one copy, behind the EM kernels
    const uint64_t S = got.subsets;
    const PackedLayout lay = packedLayout(M, S, got.list_length, got.columns, GS, got.retained);
    if (pinnedAlloc(&res->block, std::max<size_t>(lay.bytes, 64)) != hipSuccess) {
        (void) hipStreamSynchronize(st);
        setError("rpvg_hip_nested_full_subset_em: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    unsigned char * host = static_cast<unsigned char *>(res->block);
    ok(hipMemcpyAsync(host, d_packed.ptr, lay.bytes, hipMemcpyDeviceToHost, st));
    ok(waitStream(st));
    if (e != hipSuccess) {
        setError("rpvg_hip_nested_full_subset_em: %s", hipGetErrorString(e));
        return RPVG_HIP_ERR_RUNTIME;
    }
    if (*reinterpret_cast<const uint32_t *>(host + lay.merge_flags)) {
        setError("rpvg_hip_nested_full_subset_em: not taken (a path subset holds more than %u paths of one transcript (PathInfo::group_id): the "
                 "reference asserts against it, src/path_abundance_estimator.cpp:722)", GS);
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    rpvg_hip_subset_em_sets_view & v = res->sets_view;
    v.num_matrices = M;
    v.group_size = GS;
    v.subset_off = reinterpret_cast<const uint64_t *>(host + lay.subset_off);
    v.weight = reinterpret_cast<const double *>(host + lay.weight);
    v.path_off = reinterpret_cast<const uint64_t *>(host + lay.path_off);
    v.path = reinterpret_cast<const uint32_t *>(host + lay.path);
    v.col_off = reinterpret_cast<const uint64_t *>(host + lay.col_off);
    v.col_path = reinterpret_cast<const uint32_t *>(host + lay.col_path);
    v.abundances = reinterpret_cast<const double *>(host + lay.abundances);
    v.noise_count = reinterpret_cast<const double *>(host + lay.noise);
    v.total_count = reinterpret_cast<const double *>(host + lay.total);
    v.iterations = reinterpret_cast<const uint32_t *>(host + lay.iterations);
    v.retained_off = reinterpret_cast<const uint64_t *>(host + lay.retained_off);
    v.retained_rank = reinterpret_cast<const uint64_t *>(host + lay.retained_rank);
    v.retained_posterior = reinterpret_cast<const double *>(host + lay.retained_posterior);
    v.set_count = reinterpret_cast<const uint32_t *>(host + lay.set_count);
    v.cluster_noise_count = reinterpret_cast<const double *>(host + lay.cluster_noise);
    v.set_size = reinterpret_cast<const uint32_t *>(host + lay.set_size);
    v.set_member = reinterpret_cast<const uint32_t *>(host + lay.set_member);
    v.set_posterior = reinterpret_cast<const double *>(host + lay.set_posterior);
    v.set_abundance = reinterpret_cast<const double *>(host + lay.set_abund);
    // (the subset side through the diploid view as well: rpvg_hip_subset_em_get serves both results; its set_* stay NULL here)
    rpvg_hip_subset_em_view & d = res->view;
    d.num_matrices = M;
    d.subset_off = v.subset_off;
    d.weight = v.weight;
    d.path_off = v.path_off;
    d.path = v.path;
    d.col_off = v.col_off;
    d.col_path = v.col_path;
    d.abundances = v.abundances;
    d.noise_count = v.noise_count;
    d.total_count = v.total_count;
    d.iterations = v.iterations;
    res->num_subsets = S;
    res->has_sets = true;
    accountEmSolve(ctx, static_cast<uint32_t>(S), v.col_off, reinterpret_cast<const uint32_t *>(host + lay.kept_rows),
                   reinterpret_cast<const uint32_t *>(host + lay.kept_entries), v.iterations);
    ctx->stats.nested_full_calls += 1;
    ctx->stats.nested_full_sets += kept.total_sets;
    ctx->stats.nested_full_retained += got.retained;
    if (ctx->keep_subset_block) res->keep(d_packed, lay, got.list_length, GS, true);  // (rpvg_hip_subset_em_keep_device)
    *result_out = res.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_nested_full_subset_em(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups,
                                              uint32_t group_size, const double * log_freq, double min_hap_prob, uint32_t max_em_its,
                                              double max_rel_em_conv, double collapse_precision, rpvg_hip_subset_em ** result_out) {
    RPVG_REQUIRE(ctx && batch && groups && result_out, "rpvg_hip_nested_full_subset_em: NULL argument");
    *result_out = nullptr;
    RPVG_REQUIRE(max_em_its > 0, "rpvg_hip_nested_full_subset_em: max_em_its must be positive");
    RPVG_REQUIRE(groups->batch == batch, "rpvg_hip_nested_full_subset_em: the matrices were built on another batch");
    const uint32_t M = groups->num_matrices;
    RPVG_REQUIRE(M == 0 || log_freq, "rpvg_hip_nested_full_subset_em: log_freq is NULL");

    // what the call does not take (the caller makes the separate calls): decided here, before anything is queued
    rpvg_subset_full::CallShape shape;
    shape.group_size = group_size;
    shape.min_hap_prob = min_hap_prob;
    shape.num_matrices = M;
    shape.columns = groups->h_num_cols.data();
    for (uint32_t m = 0; m < M; ++m) shape.max_paths = std::max(shape.max_paths, groups->h_num_paths[m]);
    shape.has_group_ids = batch->path_group_id.ptr != nullptr;
    shape.disabled = std::getenv("RPVG_HIP_NO_DEVICE_SUBSETS") != nullptr;  // (read per call: the tests take both ways)
    uint32_t which = 0;
    switch (rpvg_subset_full::refusal(shape, &which)) {
        case rpvg_subset_full::kTaken: break;
        case rpvg_subset_full::kGroupSize:
            setError("rpvg_hip_nested_full_subset_em: not taken (group size %u: the call serves 1 and 3 .. 8, rpvg_hip_nested_subset_em is the diploid call)", group_size);
            return RPVG_HIP_ERR_UNSUPPORTED;
        case rpvg_subset_full::kDisabled:
            setError("rpvg_hip_nested_full_subset_em: not taken (RPVG_HIP_NO_DEVICE_SUBSETS)");
            return RPVG_HIP_ERR_UNSUPPORTED;
        case rpvg_subset_full::kMinHapProb:
            setError("rpvg_hip_nested_full_subset_em: not taken (min_hap_prob %g admits more than %u retained sets per matrix)", min_hap_prob, kMaxSlots);
            return RPVG_HIP_ERR_UNSUPPORTED;
        case rpvg_subset_full::kNoGroupIds:
            setError("rpvg_hip_nested_full_subset_em: not taken (the batch was uploaded without path_group_id: the merge needs the transcript of every path)");
            return RPVG_HIP_ERR_UNSUPPORTED;
        case rpvg_subset_full::kTooManySets:
            setError("rpvg_hip_nested_full_subset_em: not taken (matrix %u, %u columns, has more than %llu sets of %u)", which, groups->h_num_cols[which],
                     static_cast<unsigned long long>(RPVG_HIP_FULL_MAX_SETS), group_size);
            return RPVG_HIP_ERR_UNSUPPORTED;
        case rpvg_subset_full::kTooWide:
            setError("rpvg_hip_nested_full_subset_em: not taken (a cluster with %u paths: EM vectors in global memory)", shape.max_paths);
            return RPVG_HIP_ERR_UNSUPPORTED;
    }
    std::vector<uint64_t> sets(M);
    for (uint32_t m = 0; m < M; ++m) sets[m] = rpvg_subset_full::setCount(groups->h_num_cols[m], group_size);

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    if (M == 0) {
        std::unique_ptr<rpvg_hip_subset_em> res(new (std::nothrow) rpvg_hip_subset_em());
        if (!res) {
            setError("rpvg_hip_nested_full_subset_em: out of host memory");
            return RPVG_HIP_ERR_ALLOC;
        }
        res->has_sets = true;
        res->sets_view.group_size = group_size;
        *result_out = res.release();
        return RPVG_HIP_OK;
    }
    RetainedSets kept;
    std::vector<std::unique_ptr<GroupFullLaunch> > launches;  // (their small arrays live until the stream has been waited for)
    DeviceBuffer<double> d_posterior;
    int rc = queueEnumerationAndRetain(ctx, groups, group_size, log_freq, min_hap_prob, sets, kept, launches, d_posterior);
    if (rc != RPVG_HIP_OK) {
        (void) hipStreamSynchronize(ctx->stream);
        return rc;
    }
    bool did_not_fit = false;
    rc = nestedFullAttempt(ctx, batch, groups, group_size, min_hap_prob, max_em_its, max_rel_em_conv, collapse_precision, kept, shape.max_paths,
                           result_out, &did_not_fit);
    if (rc == RPVG_HIP_ERR_UNSUPPORTED && did_not_fit) {
        // the retained sets are on the device (sorted by the first attempt's select, which sorts them again to the same order): select,
        // expand and solve once more with the capacities the first attempt reported
        static const bool trace = std::getenv("RPVG_AMD_TRACE") != nullptr;
        if (trace) std::fprintf(stderr, "[rpvg_hip trace]   full subset em: second attempt (%s)\n", rpvg_hip_last_error());
        rc = nestedFullAttempt(ctx, batch, groups, group_size, min_hap_prob, max_em_its, max_rel_em_conv, collapse_precision, kept, shape.max_paths,
                               result_out, &did_not_fit);
    }
    (void) hipStreamSynchronize(ctx->stream);  // (every path above has waited already; the buffers go back to the pool here)
    return rc;
}

extern "C" int rpvg_hip_subset_em_get_sets(const rpvg_hip_subset_em * result, rpvg_hip_subset_em_sets_view * view_out) {
    RPVG_REQUIRE(result && view_out, "rpvg_hip_subset_em_get_sets: NULL argument");
    RPVG_REQUIRE(result->has_sets, "rpvg_hip_subset_em_get_sets: the result is the diploid call's (rpvg_hip_subset_em_get)");
    *view_out = result->sets_view;
    view_out->num_matrices = result->num_matrices;
    return RPVG_HIP_OK;
}

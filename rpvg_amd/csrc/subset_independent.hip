// Independent haplotype inference from the posteriors to the merged estimates without a host round trip (gfx950): group sizes 1 .. 8.
//
// NestedPathAbundanceEstimator::inferAbundancesIndependentGroups (src/path_abundance_estimator.cpp:356-426) with exact posteriors is
//   calculatePathGroupPosteriorsBounded / Full   per transcript                      (bounded_search.hip, group_full.hip: queued here)
//   sampleGroupPathIndices                       :548-567, S draws per transcript     <- indepDistKernel + indepDrawKernel
//   the samples sorted and counted               :414-422                             <- indepSubsetKernel
//   inferPathSubsetAbundance, per subset         :625-671                             (indepExpandKernel, then em_sparse.hip)
//   the posterior-weighted merge                 :702-749                             (fullMergeKernel, subset_full.hip)
// The unit is the cluster; its transcripts are consecutive matrices.  A transcript with fewer than two sets draws nothing, every
// other one takes exactly two generator words per sample: drawing transcript d of a cluster owns the words [2 S d, 2 S (d + 1)) of
// the cluster's stream, so every draw knows its words before any draw is made.
//   indepDistKernel     one wavefront per transcript: the construction of std::discrete_distribution (gibbs_streams.hpp) — the sum,
//                       the quotients and the partial sums as chains in index order; the lanes stage 64 weights at a time, lane 0 runs
//                       the chain over them
//   indepDrawKernel     one workgroup per cluster: the drawing transcripts numbered (prefix over "has at least two sets"), the
//                       generator's state in LDS (the untempered next 624 outputs), advanced a block of 624 words at a time in three
//                       steps; the 312 draws of a block are made while it is in LDS: thread t takes the words 2t and 2t + 1, bisects
//                       the partial sums of transcript n / S and writes the set into draw[slot n % S][transcript].  No stream is stored.
//   indepSubsetKernel   one workgroup per cluster: checks that the transcripts' columns partition the cluster's paths by
//                       path_group_id; every sample's path list (group_size paths per transcript, sorted: transcripts interleave);
//                       the samples sorted by their lists in LDS (whole lists are compared: nothing is merged on a hash), runs of
//                       equal lists counted, weights from the table of chained additions (subset_independent_plan.hpp), the
//                       `weight >= min_hap_prob` check (:627-630), subsets in lexicographic order of their lists
//   subsetOffsetsKernel, packResultsKernel   subset_pack.hpp, unchanged
//   indepExpandKernel   the lists and distinct paths of the retained subsets into the EM problem list
//   indepPackExtraKernel   sample counts, words consumed and generator states behind the packed block

#include "common.hpp"
#include "gibbs_streams.hpp"
#include "subset_independent_plan.hpp"
#include "subset_pack.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

using namespace rpvg_hip_detail;

namespace {

using rpvg_subset_independent::kMaxSamples;
using rpvg_subset_independent::kStateWords;
constexpr uint32_t kNone = 0xffffffffu;

// where the call's own arrays sit behind the packed block of subset_pack.hpp (64-byte aligned)
struct ExtraLayout {
    size_t sample_count, words, state, bytes;
};
__host__ __device__ inline ExtraLayout extraLayout(const size_t packed_bytes, const uint64_t subsets, const uint64_t units) {
    ExtraLayout x;
    size_t at = (packed_bytes + 63) & ~static_cast<size_t>(63);
    auto place = [&](const size_t bytes) {
        const size_t here = at;
        at += (bytes + 63) & ~static_cast<size_t>(63);
        return here;
    };
    x.sample_count = place(subsets * 4);
    x.words = place(units * 8);
    x.state = place(units * kStateWords * 4);
    x.bytes = at;
    return x;
}

// the posteriors of every transcript as the kernels find them: matrix m has set_count[m] sets from set_base[m] on
struct SetTable {
    const uint64_t * set_base;     // [M]
    const uint32_t * set_count;    // [M]
    const double * posterior;
    const uint32_t * pair_first;   // group size 2: the members of every kept pair
    const uint32_t * pair_second;
};

// ---- distributions -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void indepDistKernel(const uint32_t num_matrices, const SetTable sets, double * __restrict__ partial, uint32_t * __restrict__ drawing) {
    __shared__ double s_w[64];
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= num_matrices) return;
    const uint32_t n = sets.set_count[m];
    if (!rpvg_streams::discreteDraws(n)) {
        if (lane == 0) drawing[m] = 0;
        return;
    }
    const uint64_t base = sets.set_base[m];
    const double * w = sets.posterior + base;
    double * cp = partial + base;
    double sum = 0.0, run = 0.0;
    for (uint32_t c = 0; c < n; c += 64) {
        const uint32_t end = min(n, c + 64);
        if (c + lane < end) s_w[lane] = w[c + lane];
        __syncthreads();
        if (lane == 0) sum = rpvg_streams::discreteSumRange([&](const uint32_t i) { return s_w[i - c]; }, c, end, sum);
        __syncthreads();
    }
    for (uint32_t c = 0; c < n; c += 64) {
        const uint32_t end = min(n, c + 64);
        if (c + lane < end) s_w[lane] = w[c + lane];
        __syncthreads();
        if (lane == 0) {
            run = rpvg_streams::discreteCumulateRange([&](const uint32_t i) { return s_w[i - c]; }, c, end, sum, run, [&](const uint32_t i, const double v) { cp[i] = v; });
        }
        __syncthreads();
    }
    if (lane == 0) {
        cp[n - 1] = 1.0;
        drawing[m] = 1;
    }
}

// ---- stream + draw -----------------------------------------------------------------------------------------------------------
struct DrawArgs {
    uint32_t num_units, samples;
    const uint32_t * unit_mat_off;       // [K+1]
    SetTable sets;
    const double * partial;
    const uint32_t * drawing;            // [M]
    const uint32_t * generator_words;    // [K x 624]
    uint32_t * draw_list;                // [M] scratch: the drawing transcripts of every unit, from unit_mat_off[k] on
    uint32_t * draws;                    // [S x M] zero-initialised; unit k at S x unit_mat_off[k]: [slot][transcript]
    unsigned long long * words_consumed; // [K]
    uint32_t * generator_state;          // [K x 624] zero-initialised
};

constexpr int kDrawBlock = 320;                      // 312 draws per block of 624 words; the recurrence's steps are 227, 227 and 170 wide
constexpr uint32_t kDrawsPerBlock = kStateWords / 2;

__global__ __launch_bounds__(kDrawBlock) void indepDrawKernel(const DrawArgs args) {
    __shared__ uint32_t s_x[kStateWords];
    __shared__ uint32_t s_scan[kDrawBlock / 64];
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    if (k >= args.num_units) return;
    const uint32_t m0 = args.unit_mat_off[k], T = args.unit_mat_off[k + 1] - m0, S = args.samples;
    // the drawing transcripts in order: transcript draw_list[m0 + d] starts at word 2 S d
    uint32_t D = 0;
    for (uint32_t c = 0; c < T; c += kDrawBlock) {
        const uint32_t t = c + tid;
        const uint32_t flag = (t < T && args.drawing[m0 + t]) ? 1u : 0u;
        uint32_t total;
        const uint32_t before = blockExclusiveScan<kDrawBlock>(flag, total, s_scan);
        if (flag) args.draw_list[m0 + D + before] = t;
        D += total;
    }
    for (uint32_t i = tid; i < kStateWords; i += kDrawBlock) s_x[i] = rpvg_streams::mtUntemper(args.generator_words[static_cast<uint64_t>(k) * kStateWords + i]);
    __threadfence_block();
    __syncthreads();
    const unsigned long long N = static_cast<unsigned long long>(S) * D, W = 2ull * N;
    if (tid == 0) args.words_consumed[k] = W;
    const unsigned long long blocks = (W + kStateWords - 1) / kStateWords;
    uint32_t * draws = args.draws + static_cast<uint64_t>(S) * m0;
    for (unsigned long long b = 0; b < blocks; ++b) {
        if (b > 0) {  // the next 624 state words, in place: every step reads before it writes
            uint32_t v = 0;
            if (tid < rpvg_streams::kMtTail) v = rpvg_streams::mtBlockWord(s_x, tid);
            __syncthreads();
            if (tid < rpvg_streams::kMtTail) s_x[tid] = v;
            __syncthreads();
            if (tid < rpvg_streams::kMtTail) v = rpvg_streams::mtBlockWord(s_x, rpvg_streams::kMtTail + tid);
            __syncthreads();
            if (tid < rpvg_streams::kMtTail) s_x[rpvg_streams::kMtTail + tid] = v;
            __syncthreads();
            if (tid < kStateWords - 2 * rpvg_streams::kMtTail) v = rpvg_streams::mtBlockWord(s_x, 2 * rpvg_streams::kMtTail + tid);
            __syncthreads();
            if (tid < kStateWords - 2 * rpvg_streams::kMtTail) s_x[2 * rpvg_streams::kMtTail + tid] = v;
            __syncthreads();
        }
        if (W >= kStateWords) {  // the 624 state words before the generator's next output: the words [W - 624, W) of the stream
            for (uint32_t i = tid; i < kStateWords; i += kDrawBlock) {
                const unsigned long long pos = b * kStateWords + i;
                if (pos >= W - kStateWords && pos < W) args.generator_state[static_cast<uint64_t>(k) * kStateWords + (pos - (W - kStateWords))] = s_x[i];
            }
        }
        const unsigned long long n = b * kDrawsPerBlock + tid;
        if (tid < kDrawsPerBlock && n < N) {
            const uint32_t d = static_cast<uint32_t>(n / S), slot = static_cast<uint32_t>(n % S);
            const uint32_t t = args.draw_list[m0 + d];
            const uint32_t count = args.sets.set_count[m0 + t];
            const double * cp = args.partial + args.sets.set_base[m0 + t];
            const uint32_t set = rpvg_streams::discreteDraw([&](const uint32_t i) { return cp[i]; }, count, rpvg_streams::mtTemper(s_x[2 * tid]), rpvg_streams::mtTemper(s_x[2 * tid + 1]));
            draws[static_cast<uint64_t>(slot) * T + t] = min(set, count - 1);  // (a partial sum that is not a number: stay inside the sets)
        }
        __syncthreads();
    }
}

// ---- samples -> subsets ------------------------------------------------------------------------------------------------------
struct IndepSubsetArgs {
    uint32_t num_units, samples;
    const uint32_t * unit_mat_off;
    const uint32_t * unit_cluster;       // [K] kNone: a unit without transcripts
    const uint64_t * unit_path_off;      // [K+1] into `owner`
    SetTable sets;
    const uint32_t * mat_cols;           // [M]
    const uint32_t * draws;
    const uint64_t * group_off;          // [M+1]
    const uint64_t * group_path_off;
    const uint32_t * group_path;
    const uint64_t * cluster_path_off;
    const uint32_t * path_group_id;
    const uint64_t * cluster_row_off;
    const uint64_t * row_ent_off;
    const double * weight_table;         // [S+1]
    double min_hap_prob;
    uint32_t segment_rows;
    uint32_t * owner;                    // scratch, all ones: the transcript of every path of every unit
    uint32_t * mat_gid;                  // [M] scratch
    uint32_t * lists;                    // [S x M x GS]; unit k at S x unit_mat_off[k] x GS: [slot][T x GS]
    uint32_t * sub_sample;               // [S x K] per retained subset of the unit, in order: the sample that leads it
    double * slot_weight;
    uint32_t * slot_count;
    uint32_t * slot_columns;
    uint32_t * retained;                 // [K]
    MatrixTotals * totals;               // [K]
    uint32_t * bad;                      // zero-initialised: 1 + the first unit found whose columns are no partition
};

__device__ __forceinline__ void siftDown(uint32_t * a, uint32_t root, const uint32_t n) {
    const uint32_t v = a[root];
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= n) break;
        if (child + 1 < n && a[child + 1] > a[child]) ++child;
        if (a[child] <= v) break;
        a[root] = a[child];
        root = child;
    }
    a[root] = v;
}

__device__ __forceinline__ void heapSort(uint32_t * a, const uint32_t n) {
    if (n < 2) return;
    for (uint32_t start = n / 2; start-- > 0;) siftDown(a, start, n);
    for (uint32_t end = n - 1; end > 0; --end) {
        const uint32_t top = a[0];
        a[0] = a[end];
        a[end] = top;
        siftDown(a, 0, end);
    }
}

template <int GS>
__global__ __launch_bounds__(256) void indepSubsetKernel(const IndepSubsetArgs args) {
    constexpr int BLOCK = 256;
    __shared__ uint32_t s_order[kMaxSamples];
    __shared__ unsigned char s_start[kMaxSamples];
    __shared__ uint32_t s_scan[BLOCK / 64];
    __shared__ uint32_t s_bad;
    __shared__ unsigned long long s_columns;
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    if (k >= args.num_units) return;
    const uint32_t m0 = args.unit_mat_off[k], T = args.unit_mat_off[k + 1] - m0, S = args.samples;
    const uint32_t L = T * GS;
    MatrixTotals * out_totals = args.totals + k;
    if (T == 0) {
        if (tid == 0) {
            *out_totals = MatrixTotals{0, 0, 0, 0, 0, 0};
            args.retained[k] = 0;
        }
        return;
    }
    const uint32_t cluster = args.unit_cluster[k];
    const uint32_t P = static_cast<uint32_t>(args.cluster_path_off[cluster + 1] - args.cluster_path_off[cluster]);
    const uint32_t * gid = args.path_group_id + args.cluster_path_off[cluster];
    uint32_t * owner = args.owner + args.unit_path_off[k];
    if (tid == 0) {
        s_bad = 0;
        s_columns = 0;
    }
    __syncthreads();
    // every column is one path, every path of the cluster is one transcript's, and the transcripts are the path_group_ids
    for (uint32_t t = 0; t < T; ++t) {
        const uint64_t col0 = args.group_off[m0 + t];
        const uint32_t G = static_cast<uint32_t>(args.group_off[m0 + t + 1] - col0);
        if (G != args.mat_cols[m0 + t] || G == 0) s_bad = 1;
        for (uint32_t c = tid; c < G; c += BLOCK) {
            const uint64_t at = args.group_path_off[col0 + c];
            const uint32_t p = (args.group_path_off[col0 + c + 1] - at == 1) ? args.group_path[at] : kNone;
            if (p >= P) {  // (a column of no path or several, or a path outside the cluster)
                s_bad = 1;
            } else {
                if (atomicCAS(&owner[p], kNone, t) != kNone) s_bad = 1;
                if (c == 0) args.mat_gid[m0 + t] = gid[p];
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (!s_bad) {
        for (uint32_t p = tid; p < P; p += BLOCK) {
            const uint32_t t = owner[p];
            if (t == kNone || gid[p] != args.mat_gid[m0 + t]) s_bad = 1;
        }
        for (uint64_t pair = tid; pair < static_cast<uint64_t>(T) * T; pair += BLOCK) {
            const uint32_t a = static_cast<uint32_t>(pair / T), b = static_cast<uint32_t>(pair % T);
            if (a < b && args.mat_gid[m0 + a] == args.mat_gid[m0 + b]) s_bad = 1;
        }
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) {
            atomicCAS(args.bad, 0u, k + 1);
            *out_totals = MatrixTotals{0, 0, 0, 0, 0, 0};
            args.retained[k] = 0;
        }
        return;
    }
    // every sample's list: the paths of the set drawn for each transcript (one path per column), sorted over the transcripts
    const uint32_t * draws = args.draws + static_cast<uint64_t>(S) * m0;
    uint32_t * lists = args.lists + static_cast<uint64_t>(S) * m0 * GS;
    for (uint32_t s = tid; s < S; s += BLOCK) {
        uint32_t * list = lists + static_cast<uint64_t>(s) * L;
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t m = m0 + t;
            const uint32_t set = draws[static_cast<uint64_t>(s) * T + t];
            uint32_t members[GS];
            if (GS == 2) {
                const uint64_t at = args.sets.set_base[m] + set;
                members[0] = args.sets.pair_first[at];
                members[GS - 1] = args.sets.pair_second[at];
            } else {
                rpvg_subset_full::unrankSet(args.mat_cols[m], GS, set, members);
            }
            const uint64_t col0 = args.group_off[m];
            const uint32_t last_column = args.mat_cols[m] - 1;  // (a matrix whose search kept no pair: stay inside its columns)
#pragma unroll
            for (int j = 0; j < GS; ++j) list[t * GS + j] = args.group_path[args.group_path_off[col0 + min(members[j], last_column)]];
        }
        heapSort(list, L);
    }
    __threadfence_block();
    __syncthreads();
    // the samples in lexicographic order of their lists (equal lists: by sample, so that the order is one order)
    uint32_t padded = 1;
    while (padded < S) padded <<= 1;
    for (uint32_t i = tid; i < padded; i += BLOCK) s_order[i] = i < S ? i : kNone;
    __syncthreads();
    auto compare = [&](const uint32_t x, const uint32_t y) {
        const uint32_t * a = lists + static_cast<uint64_t>(x) * L, * b = lists + static_cast<uint64_t>(y) * L;
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t pa = a[j], pb = b[j];
            if (pa != pb) return pa < pb ? -1 : 1;
        }
        return 0;
    };
    auto before = [&](const uint32_t x, const uint32_t y) {
        if (x == kNone) return false;
        if (y == kNone) return true;
        const int c = compare(x, y);
        return c < 0 || (c == 0 && x < y);
    };
    for (uint32_t size = 2; size <= padded; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < padded; i += BLOCK) {
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
    // two samples are one subset iff their lists are equal (compared whole)
    for (uint32_t i = tid; i < S; i += BLOCK) s_start[i] = (i == 0 || compare(s_order[i - 1], s_order[i]) != 0) ? 1 : 0;
    __syncthreads();
    const uint64_t slot0 = static_cast<uint64_t>(S) * k;
    uint32_t n_ret = 0;
    for (uint32_t c = 0; c < S; c += BLOCK) {
        const uint32_t i = c + tid;
        uint32_t count = 0;
        double weight = 0.0;
        bool take = false;
        if (i < S && s_start[i]) {
            count = 1;
            while (i + count < S && !s_start[i + count]) ++count;
            weight = args.weight_table[count];  // `count` additions of 1 / double(S) from 0.0 (:421)
            take = weight >= args.min_hap_prob; // (:627-630)
        }
        uint32_t total;
        const uint32_t rank = n_ret + blockExclusiveScan<BLOCK>(take ? 1u : 0u, total, s_scan);
        if (take) {
            const uint32_t s = s_order[i];
            const uint32_t * list = lists + static_cast<uint64_t>(s) * L;
            uint32_t distinct = 0, previous = kNone;
            for (uint32_t j = 0; j < L; ++j) {
                distinct += (list[j] != previous) ? 1u : 0u;
                previous = list[j];
            }
            args.sub_sample[slot0 + rank] = s;
            args.slot_weight[slot0 + rank] = weight;
            args.slot_count[slot0 + rank] = count;
            args.slot_columns[slot0 + rank] = distinct;
            atomicAdd(&s_columns, static_cast<unsigned long long>(distinct));
        }
        n_ret += total;
    }
    __syncthreads();
    if (tid == 0) {
        const uint64_t r0 = args.cluster_row_off[cluster], r1 = args.cluster_row_off[cluster + 1];
        const unsigned long long rows = r1 - r0, entries = args.row_ent_off[r1] - args.row_ent_off[r0], n = n_ret;
        *out_totals = MatrixTotals{n, n * L, s_columns, n * rows, n * entries, n * ((rows + args.segment_rows - 1) / args.segment_rows)};
        args.retained[k] = n_ret;
    }
}

// ---- expand ------------------------------------------------------------------------------------------------------------------
struct IndepExpandArgs {
    uint32_t num_units, samples, group_size;
    const SubsetHeader * header;
    const MatrixTotals * totals;
    const MatrixTotals * bases;
    const uint32_t * unit_mat_off;
    const uint32_t * unit_cluster;
    const uint32_t * lists;
    const uint32_t * sub_sample;
    const double * slot_weight;
    const uint32_t * slot_count;
    const uint32_t * slot_columns;
    const uint64_t * cluster_row_off;
    const uint64_t * row_ent_off;
    uint32_t * sub_cluster;
    double * sub_weight;
    uint32_t * sub_count;
    uint64_t * path_off;
    uint32_t * path;
    uint64_t * col_off;
    uint32_t * col_path;
    uint64_t * row_base;
    uint64_t * ent_base;
    uint64_t * seg_first;
    uint32_t * item_problem;
    uint32_t segment_rows;
    uint64_t * subset_off;   // [K+1]
};

__global__ __launch_bounds__(256) void indepExpandKernel(const IndepExpandArgs args) {
    constexpr int BLOCK = 256;
    __shared__ uint32_t scratch[BLOCK / 64];
    const uint32_t k = blockIdx.x;
    if (k >= args.num_units) return;
    const MatrixTotals base = args.bases[k];
    const bool overflow = args.header->overflow != 0;
    if (threadIdx.x == 0) {
        args.subset_off[k] = overflow ? 0 : base.subsets;
        if (k + 1 == args.num_units) args.subset_off[k + 1] = overflow ? 0 : args.header->subsets;
    }
    if (overflow) return;
    const uint32_t n = static_cast<uint32_t>(args.totals[k].subsets);
    if (n == 0) return;
    const uint32_t m0 = args.unit_mat_off[k], T = args.unit_mat_off[k + 1] - m0, S = args.samples;
    const uint32_t L = T * args.group_size;
    const uint32_t * lists = args.lists + static_cast<uint64_t>(S) * m0 * args.group_size;
    const uint64_t slot0 = static_cast<uint64_t>(S) * k;
    const uint32_t cluster = args.unit_cluster[k];
    const uint64_t r0 = args.cluster_row_off[cluster], r1 = args.cluster_row_off[cluster + 1];
    const uint64_t rows = r1 - r0, entries = args.row_ent_off[r1] - args.row_ent_off[r0];
    uint64_t columns_run = base.columns;
    for (uint32_t c = 0; c < n; c += BLOCK) {
        const uint32_t r = c + threadIdx.x;
        const uint32_t cols = r < n ? args.slot_columns[slot0 + r] : 0u;
        uint32_t cols_total;
        const uint32_t cols_before = blockExclusiveScan<BLOCK>(cols, cols_total, scratch);
        if (r < n) {
            const uint64_t s = base.subsets + r;
            const uint64_t p0 = base.list_length + static_cast<uint64_t>(r) * L, c0 = columns_run + cols_before;
            args.sub_cluster[s] = cluster;
            args.sub_weight[s] = args.slot_weight[slot0 + r];
            args.sub_count[s] = args.slot_count[slot0 + r];
            args.path_off[s] = p0;
            args.col_off[s] = c0;
            args.row_base[s] = base.rows + static_cast<uint64_t>(r) * rows;
            args.ent_base[s] = base.entries + static_cast<uint64_t>(r) * entries;
            const uint64_t segments = (rows + args.segment_rows - 1) / args.segment_rows, item0 = base.segments + static_cast<uint64_t>(r) * segments;
            args.seg_first[s] = item0;
            for (uint64_t item = item0; item < item0 + segments; ++item) args.item_problem[item] = static_cast<uint32_t>(s);
            const uint32_t * list = lists + static_cast<uint64_t>(args.sub_sample[slot0 + r]) * L;
            uint32_t previous = kNone;
            uint64_t cw = c0;
            for (uint32_t j = 0; j < L; ++j) {
                const uint32_t p = list[j];
                args.path[p0 + j] = p;
                // collapsed_path_subset (:637-656): the distinct paths, ascending = the columns of the subset's EM problem
                if (p != previous) args.col_path[cw++] = p;
                previous = p;
            }
        }
        columns_run += cols_total;
    }
}

// ---- the call's own arrays behind the packed block ---------------------------------------------------------------------------
struct IndepPackArgs {
    const SubsetHeader * header;
    uint32_t num_units, group_size;
    const uint32_t * sub_count;
    const unsigned long long * words_consumed;
    const uint32_t * generator_state;
    unsigned char * packed;
};

__global__ __launch_bounds__(256) void indepPackExtraKernel(const IndepPackArgs args) {
    const SubsetHeader h = *args.header;
    if (h.overflow) return;
    const uint64_t K = args.num_units;
    const PackedLayout lay = packedLayout(K, h.subsets, h.list_length, h.columns, args.group_size, 0);
    const ExtraLayout extra = extraLayout(lay.bytes, h.subsets, K);
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x, first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    auto copy = [&](const size_t offset, const void * from, const size_t words) {  // 4-byte words
        uint32_t * to = reinterpret_cast<uint32_t *>(args.packed + offset);
        const uint32_t * src = static_cast<const uint32_t *>(from);
        for (size_t i = first; i < words; i += stride) to[i] = src[i];
    };
    copy(extra.sample_count, args.sub_count, h.subsets);
    copy(extra.words, args.words_consumed, K * 2);
    copy(extra.state, args.generator_state, K * kStateWords);
}

// the group size picks the packed layout (packResultsKernel reads it from the header); no retained-set arrays here
__global__ void indepHeaderKernel(SubsetHeader * header, const uint32_t group_size) {
    header->group_size = group_size;
    header->retained = 0;
}

// what the first stage leaves on the device: draws, lists and the retained subsets of every unit in its slots
struct IndepStage {
    uint32_t K = 0, M = 0, S = 0, GS = 0;
    std::vector<uint32_t> unit_cluster;
    uint64_t lane_rows = 0, lane_entries = 0, lane_paths = 0, max_cluster_work = 0, list_bound = 0;
    uint32_t max_paths = 0;
    DeviceBuffer<uint32_t> d_unit_mat_off, d_unit_cluster, d_draws, d_lists, d_sub_sample, d_slot_count, d_slot_columns, d_retained, d_state;
    DeviceBuffer<double> d_slot_weight;
    DeviceBuffer<unsigned long long> d_words;
    DeviceBuffer<unsigned char> d_totals;
    DeviceBuffer<uint32_t> d_bad;
};

}  // namespace

// One attempt at everything behind the retained subsets, with the capacities the context's hints give (as nestedFullAttempt).
static int independentAttempt(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups, const rpvg_hip_independent_spec * spec,
                              IndepStage & stage, rpvg_hip_subset_em ** result_out, bool * did_not_fit) {
    *did_not_fit = false;
    const uint32_t K = stage.K, GS = stage.GS, S_samples = stage.S;
    hipStream_t st = ctx->stream;
    std::unique_ptr<rpvg_hip_subset_em> res(new (std::nothrow) rpvg_hip_subset_em());
    if (!res) {
        setError("rpvg_hip_nested_independent_subset_em: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    res->num_matrices = K;
    const unsigned long long slots = static_cast<unsigned long long>(S_samples) * K;
    SubsetEmHints & hints = ctx->subset_independent_hints;
    auto planned = [](const double per_unit, const unsigned long long units, const double headroom) {
        return static_cast<unsigned long long>(std::ceil(per_unit * headroom * static_cast<double>(units)));
    };
    unsigned long long cap_subsets = std::min<unsigned long long>(slots, hints.subsets_per_matrix > 0 ? planned(hints.subsets_per_matrix, K, 1.25) + 256 : std::max<unsigned long long>(8ull * K, 16384));
    unsigned long long cap_length = std::max<unsigned long long>(planned(hints.list_per_path, stage.lane_paths, 2.0), std::max<unsigned long long>(4ull * GS * stage.lane_paths, 1u << 18));
    unsigned long long cap_rows = hints.rows_per_row > 0 ? planned(hints.rows_per_row, stage.lane_rows, 1.25) + 65536 : 8 * stage.lane_rows;
    unsigned long long cap_entries = hints.entries_per_entry > 0 ? planned(hints.entries_per_entry, stage.lane_entries, 1.25) + 65536 : 8 * stage.lane_entries;
    if (hints.retry) {
        cap_subsets = std::min<unsigned long long>(slots, std::max(cap_subsets, hints.retry_subsets + 64));
        cap_length = std::max(cap_length, hints.retry_list_length + 64);
        cap_rows = std::max(cap_rows, hints.retry_rows + 64);
        cap_entries = std::max(cap_entries, hints.retry_entries + 64);
        hints.retry = false;
    }
    cap_subsets = std::max<unsigned long long>(cap_subsets, 1);
    cap_length = std::min<unsigned long long>(cap_length, stage.list_bound + 64);  // (every sample of every unit its own subset)
    const unsigned long long cap_columns = cap_length;
    const unsigned long long cap_items = cap_rows / emFillSegmentRows() + cap_subsets;

    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    const size_t header_room = 256;
    static_assert(sizeof(SubsetHeader) <= 192, "the merge's flag word sits behind the header");
    DeviceBuffer<unsigned char> d_zero;
    ok(d_zero.alloc(header_room + emQueuesBytes()));
    if (e == hipSuccess) ok(zeroAsync(d_zero.ptr, header_room + emQueuesBytes(), st));
    SubsetHeader * header = reinterpret_cast<SubsetHeader *>(d_zero.ptr);
    uint32_t * d_merge_bad = reinterpret_cast<uint32_t *>(d_zero.ptr + 192);
    const unsigned long long * d_zero_word = reinterpret_cast<const unsigned long long *>(d_zero.ptr + 200);
    DeviceBuffer<unsigned char> d_bases, d_packed;
    ok(d_bases.alloc(sizeof(MatrixTotals) * K));
    DeviceBuffer<uint32_t> d_sub_cluster, d_sub_count, d_path, d_col_path, d_iters, d_kept_rows, d_kept_entries, d_item_problem;
    DeviceBuffer<double> d_sub_weight, d_abund, d_noise, d_total;
    DeviceBuffer<uint64_t> d_path_off, d_col_off, d_row_base, d_ent_base, d_subset_off, d_seg_first;
    ok(d_sub_cluster.alloc(cap_subsets));
    ok(d_sub_count.alloc(cap_subsets));
    ok(d_sub_weight.alloc(cap_subsets));
    ok(d_path_off.alloc(cap_subsets + 1));
    ok(d_col_off.alloc(cap_subsets + 1));
    ok(d_row_base.alloc(cap_subsets));
    ok(d_ent_base.alloc(cap_subsets));
    ok(d_subset_off.alloc(K + 1));
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
    ok(d_packed.alloc(extraLayout(packedLayout(K, cap_subsets, cap_length, cap_columns, GS, 0).bytes, cap_subsets, K).bytes));
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
        setError("rpvg_hip_nested_independent_subset_em: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        if (pinned_header) pinnedFree(pinned_header);
        if (header_here) (void) hipEventDestroy(header_here);
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    MatrixTotals * totals = reinterpret_cast<MatrixTotals *>(stage.d_totals.ptr);
    MatrixTotals * bases = reinterpret_cast<MatrixTotals *>(d_bases.ptr);

    int span = ctx->spanBegin(FAM_BUILD);
    const bool check_build = !groups->build_checked && groups->build_error_flag.ptr;
    OffsetsArgs oa;
    oa.pair_count = stage.d_retained.ptr;  // (the header's kept_pairs: the retained subsets)
    oa.log_evals = d_zero_word;
    oa.build_error = check_build ? groups->build_error_flag.ptr : nullptr;
    oa.num_matrices = K;
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
    indepHeaderKernel<<<dim3(1), dim3(1), 0, st>>>(header, GS);
    subsetOffsetsKernel<<<dim3(1), dim3(1024), 0, st>>>(oa);
    SubsetHeader * h_header = static_cast<SubsetHeader *>(pinned_header);
    ok(hipMemcpyAsync(h_header, header, sizeof(SubsetHeader), hipMemcpyDeviceToHost, st));
    ok(hipEventRecord(header_here, st));
    IndepExpandArgs ea;
    ea.num_units = K;
    ea.samples = S_samples;
    ea.group_size = GS;
    ea.header = header;
    ea.totals = totals;
    ea.bases = bases;
    ea.unit_mat_off = stage.d_unit_mat_off.ptr;
    ea.unit_cluster = stage.d_unit_cluster.ptr;
    ea.lists = stage.d_lists.ptr;
    ea.sub_sample = stage.d_sub_sample.ptr;
    ea.slot_weight = stage.d_slot_weight.ptr;
    ea.slot_count = stage.d_slot_count.ptr;
    ea.slot_columns = stage.d_slot_columns.ptr;
    ea.cluster_row_off = batch->cluster_row_off.ptr;
    ea.row_ent_off = batch->row_ent_off.ptr;
    ea.sub_cluster = d_sub_cluster.ptr;
    ea.sub_weight = d_sub_weight.ptr;
    ea.sub_count = d_sub_count.ptr;
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
    indepExpandKernel<<<dim3(K), dim3(256), 0, st>>>(ea);
    ok(hipGetLastError());
    ctx->spanEnd(span);
    ctx->stats.build_launches += 2;

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
    list.max_cols = stage.max_paths + 1;
    list.max_cluster_paths = stage.max_paths;
    list.max_cluster_work = stage.max_cluster_work;
    list.wide_capacity = 0;
    EmOutputs out{d_abund.ptr, d_noise.ptr, d_iters.ptr, d_kept_rows.ptr, d_kept_entries.ptr, d_total.ptr};
    EmSolveWork work;
    work.zeroed_queues = d_zero.ptr + header_room;
    if (e == hipSuccess) {
        const int rc = queueEmSolve(ctx, batch, list, spec->max_em_its, spec->max_rel_em_conv, out, work, spec->collapse_precision);
        if (rc != RPVG_HIP_OK) {
            (void) hipStreamSynchronize(st);
            (void) hipEventDestroy(header_here);
            pinnedFree(pinned_header);
            return rc;
        }
    }
    if (e == hipSuccess) {
        FullMergeLaunch ma;
        ma.header = header;
        ma.num_units = K;
        ma.subset_off = d_subset_off.ptr;
        ma.weight = d_sub_weight.ptr;
        ma.path_off = d_path_off.ptr;
        ma.path = d_path.ptr;
        ma.col_off = d_col_off.ptr;
        ma.col_path = d_col_path.ptr;
        ma.abundances = d_abund.ptr;
        ma.noise = d_noise.ptr;
        ma.total = d_total.ptr;
        ma.cluster = stage.d_unit_cluster.ptr;
        ma.cluster_path_off = batch->cluster_path_off.ptr;
        ma.path_group_id = batch->path_group_id.ptr;
        ma.sort_key = d_merge_key.ptr;
        ma.sort_pos = d_merge_pos.ptr;
        ma.rec_abund = d_merge_abund.ptr;
        ma.merge_bad = d_merge_bad;
        ma.packed = d_packed.ptr;
        const int merge_span = ctx->spanBegin(FAM_BUILD);
        queueFullMerge(GS, ma, st);
        IndepPackArgs xa;
        xa.header = header;
        xa.num_units = K;
        xa.group_size = GS;
        xa.sub_count = d_sub_count.ptr;
        xa.words_consumed = stage.d_words.ptr;
        xa.generator_state = stage.d_state.ptr;
        xa.packed = d_packed.ptr;
        indepPackExtraKernel<<<dim3(256), dim3(256), 0, st>>>(xa);
        ctx->spanEnd(merge_span);
        ctx->stats.build_launches += 2;
    }
    PackArgs pa;
    pa.merge_bad = d_merge_bad;
    pa.header = header;
    pa.num_matrices = K;
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
        setError("rpvg_hip_nested_independent_subset_em: %s", hipGetErrorString(e));
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
        fold(hints.subsets_per_matrix, got.subsets, K);
        fold(hints.list_per_path, got.list_length, stage.lane_paths);
        fold(hints.rows_per_row, got.rows, stage.lane_rows);
        fold(hints.entries_per_entry, got.entries, stage.lane_entries);
    }
    if (got.build_bad) {
        (void) hipStreamSynchronize(st);
        setError(got.build_bad == 2 ? "rpvg_hip_groups_build: a group lists a path twice" : "rpvg_hip_groups_build: a group refers to a path outside its cluster");
        return RPVG_HIP_ERR_INVALID;
    }
    groups->build_checked = true;
    if (got.overflow) {
        (void) hipStreamSynchronize(st);  // (the kernels behind the header saw zero problems)
        setError("rpvg_hip_nested_independent_subset_em: not taken (%llu subsets, %llu list entries, %llu rows, %llu entries: over the reserved capacity)",
                 got.subsets, got.list_length, got.rows, got.entries);
        hints.retry = true;
        hints.retry_subsets = got.subsets;
        hints.retry_list_length = std::max(got.list_length, got.columns);
        hints.retry_rows = got.rows;
        hints.retry_entries = got.entries;
        *did_not_fit = true;
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    // exactly what there is: one block, one copy, behind the EM kernels
    const uint64_t S = got.subsets;
    const PackedLayout lay = packedLayout(K, S, got.list_length, got.columns, GS, 0);
    const ExtraLayout extra = extraLayout(lay.bytes, S, K);
    if (pinnedAlloc(&res->block, std::max<size_t>(extra.bytes, 64)) != hipSuccess) {
        (void) hipStreamSynchronize(st);
        setError("rpvg_hip_nested_independent_subset_em: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    unsigned char * host = static_cast<unsigned char *>(res->block);
    uint32_t unit_bad = 0;
    ok(hipMemcpyAsync(host, d_packed.ptr, extra.bytes, hipMemcpyDeviceToHost, st));
    ok(hipMemcpyAsync(&unit_bad, stage.d_bad.ptr, sizeof(unit_bad), hipMemcpyDeviceToHost, st));
    ok(waitStream(st));
    if (e != hipSuccess) {
        setError("rpvg_hip_nested_independent_subset_em: %s", hipGetErrorString(e));
        return RPVG_HIP_ERR_RUNTIME;
    }
    if (unit_bad) {
        setError("rpvg_hip_nested_independent_subset_em: the columns of unit %u's transcripts do not partition its cluster's paths by path_group_id "
                 "(one path per column, every path of the cluster in exactly one transcript)", unit_bad - 1);
        return RPVG_HIP_ERR_INVALID;
    }
    if (*reinterpret_cast<const uint32_t *>(host + lay.merge_flags)) {
        setError("rpvg_hip_nested_independent_subset_em: not taken (a path subset holds more than %u paths of one transcript)", GS);
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    rpvg_hip_subset_em_independent_view & v = res->independent_view;
    v.num_clusters = K;
    v.group_size = GS;
    v.num_samples = S_samples;
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
    v.set_count = reinterpret_cast<const uint32_t *>(host + lay.set_count);
    v.cluster_noise_count = reinterpret_cast<const double *>(host + lay.cluster_noise);
    v.set_size = reinterpret_cast<const uint32_t *>(host + lay.set_size);
    v.set_member = reinterpret_cast<const uint32_t *>(host + lay.set_member);
    v.set_posterior = reinterpret_cast<const double *>(host + lay.set_posterior);
    v.set_abundance = reinterpret_cast<const double *>(host + lay.set_abund);
    v.sample_count = reinterpret_cast<const uint32_t *>(host + extra.sample_count);
    v.words_consumed = reinterpret_cast<const uint64_t *>(host + extra.words);
    v.generator_state = reinterpret_cast<const uint32_t *>(host + extra.state);
    // (the subset side through the diploid view as well: rpvg_hip_subset_em_get serves every result; its set_* stay NULL here)
    rpvg_hip_subset_em_view & d = res->view;
    d.num_matrices = K;
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
    res->has_independent = true;
    accountEmSolve(ctx, static_cast<uint32_t>(S), v.col_off, reinterpret_cast<const uint32_t *>(host + lay.kept_rows),
                   reinterpret_cast<const uint32_t *>(host + lay.kept_entries), v.iterations);
    unsigned long long draws = 0;
    for (uint32_t k = 0; k < K; ++k) draws += v.words_consumed[k] / rpvg_subset_independent::kWordsPerDraw;
    ctx->independent_stats.calls_completed += 1;
    ctx->independent_stats.draws += draws;
    ctx->independent_stats.subsets += S;
    if (ctx->keep_subset_block) res->keep(d_packed, lay, got.list_length, GS, true);  // (rpvg_hip_subset_em_keep_device)
    *result_out = res.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_nested_independent_subset_em(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups,
                                                     const rpvg_hip_independent_spec * spec, rpvg_hip_subset_em ** result_out) {
    RPVG_REQUIRE(ctx && batch && groups && spec && result_out, "rpvg_hip_nested_independent_subset_em: NULL argument");
    *result_out = nullptr;
    RPVG_REQUIRE(spec->max_em_its > 0, "rpvg_hip_nested_independent_subset_em: max_em_its must be positive");
    RPVG_REQUIRE(groups->batch == batch, "rpvg_hip_nested_independent_subset_em: the matrices were built on another batch");
    const uint32_t K = spec->num_clusters, M = groups->num_matrices, GS = spec->group_size;
    RPVG_REQUIRE(K == 0 || (spec->matrix_off && spec->generator_words), "rpvg_hip_nested_independent_subset_em: matrix_off or generator_words is NULL");
    RPVG_REQUIRE(K > 0 || M == 0, "rpvg_hip_nested_independent_subset_em: %u matrices and no unit", M);
    for (uint32_t k = 0; k < K; ++k) {
        RPVG_REQUIRE(spec->matrix_off[k] <= spec->matrix_off[k + 1], "rpvg_hip_nested_independent_subset_em: matrix_off decreases at unit %u", k);
    }
    RPVG_REQUIRE(K == 0 || (spec->matrix_off[0] == 0 && spec->matrix_off[K] == M), "rpvg_hip_nested_independent_subset_em: matrix_off does not span the %u matrices", M);

    // what the call does not take (the caller takes the separate route): decided here, before anything is queued
    rpvg_subset_independent::CallShape shape;
    shape.group_size = GS;
    shape.min_hap_prob = spec->min_hap_prob;
    shape.num_matrices = M;
    shape.columns = groups->h_num_cols.data();
    for (uint32_t m = 0; m < M; ++m) shape.max_paths = std::max(shape.max_paths, groups->h_num_paths[m]);
    shape.has_group_ids = batch->path_group_id.ptr != nullptr;
    shape.disabled = std::getenv("RPVG_HIP_NO_DEVICE_SUBSETS") != nullptr;  // (read per call: the tests take both ways)
    uint32_t which = 0;
    const rpvg_subset_independent::Refusal refused = rpvg_subset_independent::refusal(shape, &which);
    if (refused != rpvg_subset_independent::kTaken) {
        setError("rpvg_hip_nested_independent_subset_em: not taken (%s; group size %u, min_hap_prob %g, matrix %u)", rpvg_subset_independent::refusalText(refused), GS,
                 spec->min_hap_prob, which);
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    RPVG_REQUIRE(M == 0 || (GS == 2 ? (spec->column_counts || groups->d_column_counts) : spec->log_freq != nullptr),
                 "rpvg_hip_nested_independent_subset_em: %s is NULL", GS == 2 ? "column_counts" : "log_freq");

    IndepStage stage;
    stage.K = K;
    stage.M = M;
    stage.GS = GS;
    stage.S = rpvg_subset_independent::numSamples(spec->min_hap_prob);
    const uint32_t S = stage.S;
    stage.unit_cluster.assign(K, kNone);
    std::vector<uint64_t> unit_path_off(K + 1, 0);
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t m0 = spec->matrix_off[k], m1 = spec->matrix_off[k + 1];
        unit_path_off[k + 1] = unit_path_off[k];
        if (m0 == m1) continue;
        const uint32_t cluster = groups->h_cluster[m0];
        for (uint32_t m = m0 + 1; m < m1; ++m) {
            RPVG_REQUIRE(groups->h_cluster[m] == cluster, "rpvg_hip_nested_independent_subset_em: the matrices of unit %u are not of one cluster (matrix %u: cluster %u, matrix %u: cluster %u)",
                         k, m0, cluster, m, groups->h_cluster[m]);
        }
        stage.unit_cluster[k] = cluster;
        unit_path_off[k + 1] += groups->h_num_paths[m0];
        stage.lane_rows += batch->h_cluster_row_off[cluster + 1] - batch->h_cluster_row_off[cluster];
        stage.lane_entries += batch->h_cluster_ent_off[cluster + 1] - batch->h_cluster_ent_off[cluster];
        stage.lane_paths += groups->h_num_paths[m0];
        stage.max_cluster_work = std::max<uint64_t>(stage.max_cluster_work, (batch->h_cluster_row_off[cluster + 1] - batch->h_cluster_row_off[cluster]) +
                                                                                (batch->h_cluster_ent_off[cluster + 1] - batch->h_cluster_ent_off[cluster]));
    }
    stage.max_paths = shape.max_paths;
    stage.list_bound = static_cast<uint64_t>(S) * M * GS;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<rpvg_hip_subset_em> empty(new (std::nothrow) rpvg_hip_subset_em());
    if (!empty) {
        setError("rpvg_hip_nested_independent_subset_em: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    if (K == 0) {
        empty->has_independent = true;
        empty->independent_view.group_size = GS;
        empty->independent_view.num_samples = S;
        *result_out = empty.release();
        return RPVG_HIP_OK;
    }

    // ---- the posteriors of every transcript, left on the device ----
    PairSearchWork search;
    std::vector<std::unique_ptr<GroupFullLaunch> > launches;
    DeviceBuffer<double> d_posterior, d_partial, d_weight_table;
    DeviceBuffer<uint64_t> d_set_base, d_unit_path_off;
    DeviceBuffer<uint32_t> d_set_count, d_drawing, d_draw_list, d_owner, d_mat_gid;
    SetTable sets{nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t total_sets = 0;
    bool searched = false;
    if (M > 0 && GS == 2) {
        const int rc = queuePairSearch(ctx, groups, spec->column_counts, spec->min_hap_prob, search);
        if (rc != RPVG_HIP_OK) return rc;
        searched = true;
        sets = SetTable{search.d_pair_cap_off.ptr, search.d_tail.ptr, search.d_out_value.ptr, search.d_out_first.ptr, search.d_out_second.ptr};
        total_sets = search.plan.pair_cap_off[M];
    } else if (M > 0) {
        std::vector<uint64_t> set_count64(M), set_base(M);
        std::vector<uint32_t> set_count(M), matrix(M);
        for (uint32_t m = 0; m < M; ++m) {
            set_count64[m] = rpvg_subset_full::setCount(groups->h_num_cols[m], GS);
            set_count[m] = static_cast<uint32_t>(set_count64[m]);
            set_base[m] = total_sets;
            total_sets += set_count64[m];
            matrix[m] = m;
        }
        RPVG_HIP_CHECK(d_posterior.alloc(total_sets));
        RPVG_HIP_CHECK(d_set_base.upload(set_base.data(), M, st));
        RPVG_HIP_CHECK(d_set_count.upload(set_count.data(), M, st));
        RPVG_HIP_CHECK(groups->waitCollapse(st));
        uint64_t lf_first = 0;
        for (uint32_t first = 0; first < M;) {  // cut as rpvg_hip_group_full_posteriors cuts them: one set of kernels, one order of additions
            const uint32_t end = rpvg_subset_full::chunkEnd(set_count64.data(), first, M);
            launches.emplace_back(new GroupFullLaunch());
            GroupFullLaunch & work = *launches.back();
            const int rc = queueGroupFullLaunch(ctx, groups, matrix.data() + first, end - first, set_count64.data() + first, GS, spec->log_freq + lf_first, work,
                                                d_posterior.ptr + set_base[first]);
            if (rc != RPVG_HIP_OK) {
                (void) hipStreamSynchronize(st);
                return rc;
            }
            lf_first += work.lf_count;
            first = end;
        }
        sets = SetTable{d_set_base.ptr, d_set_count.ptr, d_posterior.ptr, nullptr, nullptr};
    }

    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    std::vector<double> weight_table(static_cast<size_t>(S) + 1);
    rpvg_subset_independent::weightTable(S, weight_table.data());
    const uint64_t draw_words = static_cast<uint64_t>(S) * M;
    ok(d_partial.alloc(std::max<uint64_t>(total_sets, 1)));
    ok(d_drawing.alloc(std::max<uint32_t>(M, 1)));
    ok(d_draw_list.alloc(std::max<uint32_t>(M, 1)));
    ok(d_mat_gid.alloc(std::max<uint32_t>(M, 1)));
    ok(d_owner.alloc(std::max<uint64_t>(unit_path_off[K], 1)));
    ok(stage.d_draws.alloc(std::max<uint64_t>(draw_words, 1)));
    ok(stage.d_lists.alloc(std::max<uint64_t>(stage.list_bound, 1)));
    ok(stage.d_words.alloc(K));
    ok(stage.d_state.alloc(static_cast<uint64_t>(K) * kStateWords));
    ok(stage.d_bad.alloc(1));
    ok(stage.d_retained.alloc(K));
    ok(stage.d_totals.alloc(sizeof(MatrixTotals) * K));
    const uint64_t slots = static_cast<uint64_t>(S) * K;
    ok(stage.d_sub_sample.alloc(slots));
    ok(stage.d_slot_weight.alloc(slots));
    ok(stage.d_slot_count.alloc(slots));
    ok(stage.d_slot_columns.alloc(slots));
    DeviceBuffer<uint32_t> d_words_in;
    if (e == hipSuccess) ok(d_words_in.upload(spec->generator_words, static_cast<uint64_t>(K) * kStateWords, st));
    if (e == hipSuccess) ok(stage.d_unit_mat_off.upload(spec->matrix_off, K + 1, st));
    if (e == hipSuccess) ok(stage.d_unit_cluster.upload(stage.unit_cluster.data(), K, st));
    if (e == hipSuccess) ok(d_unit_path_off.upload(unit_path_off.data(), K + 1, st));
    if (e == hipSuccess) ok(d_weight_table.upload(weight_table.data(), weight_table.size(), st));
    if (e == hipSuccess) ok(zeroAsync(stage.d_draws.ptr, std::max<uint64_t>(draw_words, 1) * 4, st));
    if (e == hipSuccess) ok(zeroAsync(stage.d_state.ptr, static_cast<size_t>(K) * kStateWords * 4, st));
    if (e == hipSuccess) ok(zeroAsync(stage.d_bad.ptr, 4, st));
    if (e == hipSuccess) ok(hipMemsetAsync(d_owner.ptr, 0xff, std::max<uint64_t>(unit_path_off[K], 1) * 4, st));
    if (e != hipSuccess) {
        if (searched) leavePairSearch(ctx);
        (void) hipStreamSynchronize(st);
        setError("rpvg_hip_nested_independent_subset_em: %s", hipGetErrorString(e));
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    ctx->stats.h2d_bytes += static_cast<double>(K) * (kStateWords * 4 + 16) + static_cast<double>(M) * 12;

    int span = ctx->spanBegin(FAM_BUILD);
    if (M > 0) indepDistKernel<<<dim3(M), dim3(64), 0, st>>>(M, sets, d_partial.ptr, d_drawing.ptr);
    DrawArgs da;
    da.num_units = K;
    da.samples = S;
    da.unit_mat_off = stage.d_unit_mat_off.ptr;
    da.sets = sets;
    da.partial = d_partial.ptr;
    da.drawing = d_drawing.ptr;
    da.generator_words = d_words_in.ptr;
    da.draw_list = d_draw_list.ptr;
    da.draws = stage.d_draws.ptr;
    da.words_consumed = stage.d_words.ptr;
    da.generator_state = stage.d_state.ptr;
    indepDrawKernel<<<dim3(K), dim3(kDrawBlock), 0, st>>>(da);
    IndepSubsetArgs sa;
    sa.num_units = K;
    sa.samples = S;
    sa.unit_mat_off = stage.d_unit_mat_off.ptr;
    sa.unit_cluster = stage.d_unit_cluster.ptr;
    sa.unit_path_off = d_unit_path_off.ptr;
    sa.sets = sets;
    sa.mat_cols = groups->mat_cols.ptr;
    sa.draws = stage.d_draws.ptr;
    sa.group_off = groups->d_group_off;
    sa.group_path_off = groups->d_group_path_off;
    sa.group_path = groups->d_group_path;
    sa.cluster_path_off = batch->cluster_path_off.ptr;
    sa.path_group_id = batch->path_group_id.ptr;
    sa.cluster_row_off = batch->cluster_row_off.ptr;
    sa.row_ent_off = batch->row_ent_off.ptr;
    sa.weight_table = d_weight_table.ptr;
    sa.min_hap_prob = spec->min_hap_prob;
    sa.segment_rows = emFillSegmentRows();
    sa.owner = d_owner.ptr;
    sa.mat_gid = d_mat_gid.ptr;
    sa.lists = stage.d_lists.ptr;
    sa.sub_sample = stage.d_sub_sample.ptr;
    sa.slot_weight = stage.d_slot_weight.ptr;
    sa.slot_count = stage.d_slot_count.ptr;
    sa.slot_columns = stage.d_slot_columns.ptr;
    sa.retained = stage.d_retained.ptr;
    sa.totals = reinterpret_cast<MatrixTotals *>(stage.d_totals.ptr);
    sa.bad = stage.d_bad.ptr;
    switch (GS) {
        case 1: indepSubsetKernel<1><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 2: indepSubsetKernel<2><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 3: indepSubsetKernel<3><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 4: indepSubsetKernel<4><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 5: indepSubsetKernel<5><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 6: indepSubsetKernel<6><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        case 7: indepSubsetKernel<7><<<dim3(K), dim3(256), 0, st>>>(sa); break;
        default: indepSubsetKernel<8><<<dim3(K), dim3(256), 0, st>>>(sa); break;
    }
    ok(hipGetLastError());
    ctx->spanEnd(span);
    ctx->stats.build_launches += 3;
    // (the next search of another context starts behind this call's small kernels, not behind its search alone)
    if (searched) leavePairSearch(ctx);
    if (e != hipSuccess) {
        (void) hipStreamSynchronize(st);
        setError("rpvg_hip_nested_independent_subset_em: %s", hipGetErrorString(e));
        return RPVG_HIP_ERR_RUNTIME;
    }

    bool did_not_fit = false;
    int rc = independentAttempt(ctx, batch, groups, spec, stage, result_out, &did_not_fit);
    if (rc == RPVG_HIP_ERR_UNSUPPORTED && did_not_fit) {
        // draws, lists and retained subsets are on the device: offsets, expand and solve once more with what the first attempt reported
        static const bool trace = std::getenv("RPVG_AMD_TRACE") != nullptr;
        if (trace) std::fprintf(stderr, "[rpvg_hip trace]   independent subset em: second attempt (%s)\n", rpvg_hip_last_error());
        rc = independentAttempt(ctx, batch, groups, spec, stage, result_out, &did_not_fit);
    }
    if (rc == RPVG_HIP_OK && searched) {  // the search's counters: kept pairs per matrix and the evaluations (statistics)
        std::vector<uint32_t> tail(search.tail_words);
        if (hipMemcpyAsync(tail.data(), search.d_tail.ptr, tail.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess && waitStream(st) == hipSuccess) {
            unsigned long long log_evals = 0, kept = 0;
            std::memcpy(&log_evals, tail.data() + search.evals_word, sizeof(log_evals));
            for (uint32_t m = 0; m < M; ++m) kept += tail[m];
            accountPairSearch(ctx, groups, search, log_evals, kept);
        }
    }
    if (rc == RPVG_HIP_OK && spec->keep_draws) {
        rpvg_hip_subset_em * res = *result_out;
        res->draws.assign(draw_words, 0);
        res->draw_off.assign(K + 1, 0);
        for (uint32_t k = 0; k <= K; ++k) res->draw_off[k] = static_cast<uint64_t>(S) * spec->matrix_off[k];
        if (draw_words && (hipMemcpyAsync(res->draws.data(), stage.d_draws.ptr, draw_words * 4, hipMemcpyDeviceToHost, st) != hipSuccess || waitStream(st) != hipSuccess)) {
            rpvg_hip_subset_em_free(res);
            *result_out = nullptr;
            setError("rpvg_hip_nested_independent_subset_em: the draws could not be copied");
            rc = RPVG_HIP_ERR_RUNTIME;
        }
    }
    (void) hipStreamSynchronize(st);  // (every path above has waited already; the buffers go back to the pool here)
    return rc;
}

extern "C" int rpvg_hip_subset_em_get_independent(const rpvg_hip_subset_em * result, rpvg_hip_subset_em_independent_view * view_out) {
    RPVG_REQUIRE(result && view_out, "rpvg_hip_subset_em_get_independent: NULL argument");
    RPVG_REQUIRE(result->has_independent, "rpvg_hip_subset_em_get_independent: the result is another call's");
    *view_out = result->independent_view;
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_independent_draws_get(const rpvg_hip_subset_em * result, uint32_t unit, uint32_t * draws_out) {
    RPVG_REQUIRE(result && draws_out, "rpvg_hip_independent_draws_get: NULL argument");
    RPVG_REQUIRE(result->has_independent && !result->draw_off.empty(), "rpvg_hip_independent_draws_get: the call did not keep its draws (keep_draws)");
    RPVG_REQUIRE(unit + 1 < result->draw_off.size(), "rpvg_hip_independent_draws_get: unit %u of %zu", unit, result->draw_off.size() - 1);
    const uint64_t first = result->draw_off[unit], count = result->draw_off[unit + 1] - first;
    if (count) std::memcpy(draws_out, result->draws.data() + first, count * sizeof(uint32_t));
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_independent_limits(rpvg_independent_limits * limits_out) {
    if (!limits_out) return;
    limits_out->max_group_size = rpvg_subset_independent::kMaxGroupSize;
    limits_out->max_samples = rpvg_subset_independent::kMaxSamples;
    limits_out->max_transcript_sets = rpvg_subset_independent::kMaxTranscriptSets;
    limits_out->words_per_draw = rpvg_subset_independent::kWordsPerDraw;
    limits_out->state_words = rpvg_subset_independent::kStateWords;
    limits_out->max_work_bytes = rpvg_subset_independent::kMaxWorkBytes;
}

extern "C" int rpvg_hip_independent_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_independent_stats * stats_out) {
    RPVG_REQUIRE(ctx && stats_out, "rpvg_hip_independent_stats_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    *stats_out = ctx->independent_stats;
    return RPVG_HIP_OK;
}

// What the two nested calls share (subset_em.hip: diploid search -> subsets -> EM -> merge; subset_full.hip: the same from the full
// enumeration of the sets of ploidy 1 and 3 .. 8): the per-matrix totals and their prefix sums against the reserved capacities
// (subsetOffsetsKernel), the header the host reads while the EM runs, the packed block of results and the kernel that fills it
// (packResultsKernel; the layout is rpvg_subset_full::packedLayout, subset_full_plan.hpp), and the result object.  One copy of each.
#pragma once

#include "common.hpp"
#include "subset_full_plan.hpp"
#include "subset_result.hpp"

using rpvg_subset_full::PackedLayout;
using rpvg_subset_full::packedLayout;
using namespace rpvg_hip_detail;

namespace rpvg_hip_detail {
// fullMergeKernel<GS> (subset_full.hip) queued from another file: its arguments (header: the call's SubsetHeader on the device), with
// units — matrices there, clusters in subset_independent.hip — that each have a cluster and a run of subsets
struct FullMergeLaunch {
    const void * header;
    uint32_t num_units;
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
    uint32_t * sort_key;
    uint32_t * sort_pos;
    double * rec_abund;
    uint32_t * merge_bad;
    unsigned char * packed;
};
void queueFullMerge(uint32_t group_size, const FullMergeLaunch & launch, hipStream_t st);
}  // namespace rpvg_hip_detail

namespace {

struct MatrixTotals {  // what subsetOffsetsKernel adds up over the matrices
    unsigned long long subsets, list_length, columns, rows, entries, segments;
};

struct SubsetHeader {  // device -> host, one small copy
    unsigned long long subsets, list_length, columns, rows, entries, segments;  // totals (what the capacities must hold)
    unsigned long long overflow;    // != 0: something did not fit (num_problems is 0 then, nothing behind runs)
    uint32_t num_problems;
    uint32_t num_items;             // row segments of all problems (em_sparse.hip: the work items of the compaction)
    uint32_t build_bad, pad;             // validity flag of the matrices' build (they were built without a host synchronisation)
    unsigned long long select_overflow;  // matrices with more selected diplotypes than kMaxSelected
    unsigned long long log_evals, kept_pairs;  // the search's counters (statistics)
    uint32_t big_count, pad2;        // matrices with more kept pairs than the one-wave select kernel takes
    // subset_full.hip (zero in the diploid call): the group size, which picks the packed layout, and the retained sets of all matrices
    uint32_t group_size, pad3;
    unsigned long long retained;
};

template <int BLOCK>
__device__ __forceinline__ uint32_t blockExclusiveScan(const uint32_t v, uint32_t & total, uint32_t * scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        if (w < wave) before += scratch[w];
        all += scratch[w];
    }
    total = all;
    return before + incl - v;
}

struct OffsetsArgs {
    const uint32_t * pair_count;      // [M] (the search's tail words)
    const unsigned long long * log_evals;
    const uint32_t * build_error;     // null: already checked
    uint32_t num_matrices;
    const MatrixTotals * totals;   // [M]
    MatrixTotals * bases;          // [M] exclusive prefix
    SubsetHeader * header;
    unsigned long long cap_subsets, cap_length, cap_columns, cap_rows, cap_entries, cap_items;
    uint64_t * seg_first;          // [cap_subsets + 1]
    uint64_t * path_off;           // [cap_subsets + 1]: the terminal entries are written here
    uint64_t * col_off;
};

__global__ __launch_bounds__(1024) void subsetOffsetsKernel(const OffsetsArgs args) {
    __shared__ MatrixTotals sums[1024];
    const uint32_t M = args.num_matrices;
    const uint32_t per = (M + 1023) / 1024;
    const uint32_t lo = min(M, threadIdx.x * per), hi = min(M, lo + per);
    MatrixTotals mine{0, 0, 0, 0, 0, 0};
    unsigned long long my_pairs = 0;
    for (uint32_t m = lo; m < hi; ++m) {
        my_pairs += args.pair_count[m];
        const MatrixTotals t = args.totals[m];
        mine.subsets += t.subsets;
        mine.list_length += t.list_length;
        mine.columns += t.columns;
        mine.rows += t.rows;
        mine.entries += t.entries;
        mine.segments += t.segments;
    }
    sums[threadIdx.x] = mine;
    if (my_pairs) atomicAdd(&args.header->kept_pairs, my_pairs);
    __syncthreads();
    for (uint32_t step = 1; step < 1024; step <<= 1) {
        MatrixTotals add{0, 0, 0, 0, 0, 0};
        if (threadIdx.x >= step) add = sums[threadIdx.x - step];
        __syncthreads();
        MatrixTotals & s = sums[threadIdx.x];
        s.subsets += add.subsets;
        s.list_length += add.list_length;
        s.columns += add.columns;
        s.rows += add.rows;
        s.entries += add.entries;
        s.segments += add.segments;
        __syncthreads();
    }
    MatrixTotals run = sums[threadIdx.x];
    run.subsets -= mine.subsets;
    run.list_length -= mine.list_length;
    run.columns -= mine.columns;
    run.rows -= mine.rows;
    run.entries -= mine.entries;
    run.segments -= mine.segments;
    for (uint32_t m = lo; m < hi; ++m) {
        args.bases[m] = run;
        const MatrixTotals t = args.totals[m];
        run.subsets += t.subsets;
        run.list_length += t.list_length;
        run.columns += t.columns;
        run.rows += t.rows;
        run.entries += t.entries;
        run.segments += t.segments;
    }
    if (threadIdx.x == 1023) {
        const MatrixTotals all = sums[1023];
        SubsetHeader * h = args.header;
        h->subsets = all.subsets;
        h->list_length = all.list_length;
        h->columns = all.columns;
        h->rows = all.rows;
        h->entries = all.entries;
        h->segments = all.segments;
        const bool fits = h->select_overflow == 0 && all.subsets <= args.cap_subsets && all.list_length <= args.cap_length &&
                          all.columns <= args.cap_columns && all.rows <= args.cap_rows && all.entries <= args.cap_entries &&
                          all.segments <= args.cap_items && all.subsets < 0xffffffffull && all.segments < 0xffffffffull;
        h->overflow = fits ? 0ull : 1ull;
        h->num_problems = fits ? static_cast<uint32_t>(all.subsets) : 0u;
        h->num_items = fits ? static_cast<uint32_t>(all.segments) : 0u;
        h->log_evals = *args.log_evals;
        h->build_bad = args.build_error ? *args.build_error : 0u;
        if (fits) {
            args.path_off[all.subsets] = all.list_length;
            args.col_off[all.subsets] = all.columns;
            args.seg_first[all.subsets] = all.segments;
        }
    }
}

struct PackArgs {
    const SubsetHeader * header;
    uint32_t num_matrices;
    const uint64_t * subset_off;
    const double * weight;
    const uint64_t * path_off;
    const uint64_t * col_off;
    const double * abundances;
    const double * noise;
    const double * total;
    const uint32_t * path;
    const uint32_t * col_path;
    const uint32_t * iterations;
    const uint32_t * kept_rows;
    const uint32_t * kept_entries;
    const uint32_t * merge_bad;  // null: no merge on the device
    unsigned char * packed;
};

__global__ __launch_bounds__(256) void packResultsKernel(const PackArgs args) {
    const SubsetHeader h = *args.header;
    if (h.overflow) return;
    const uint64_t M = args.num_matrices, S = h.subsets, L = h.list_length, C = h.columns;
    const PackedLayout lay = packedLayout(M, S, L, C, h.group_size, h.retained);
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x, first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    auto copy = [&](const size_t offset, const void * from, const size_t words) {  // 4-byte words
        uint32_t * to = reinterpret_cast<uint32_t *>(args.packed + offset);
        const uint32_t * src = static_cast<const uint32_t *>(from);
        for (size_t i = first; i < words; i += stride) to[i] = src[i];
    };
    copy(lay.subset_off, args.subset_off, (M + 1) * 2);
    copy(lay.weight, args.weight, S * 2);
    copy(lay.path_off, args.path_off, (S + 1) * 2);
    copy(lay.col_off, args.col_off, (S + 1) * 2);
    copy(lay.abundances, args.abundances, C * 2);
    copy(lay.noise, args.noise, S * 2);
    copy(lay.total, args.total, S * 2);
    copy(lay.path, args.path, L);
    copy(lay.col_path, args.col_path, C);
    copy(lay.iterations, args.iterations, S);
    copy(lay.kept_rows, args.kept_rows, S);
    copy(lay.kept_entries, args.kept_entries, S);
    if (args.merge_bad && first == 0) *reinterpret_cast<uint32_t *>(args.packed + lay.merge_flags) = *args.merge_bad;
}

}  // namespace

// the result object: subset_result.hpp

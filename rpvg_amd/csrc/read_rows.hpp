// What read_rows.hip (the per-read kernels, the pack, the entry points) and rows_merge.hip (the sort and merge of a cluster's
// rows) share: the resident rows, the padded per-read slices the kernels of both files read, and the merge stage itself.
#ifndef RPVG_HIP_READ_ROWS_HPP
#define RPVG_HIP_READ_ROWS_HPP

#include "alignments.hpp"
#include "common.hpp"

// Device-resident rows in the grouped layout of rpvg_cluster_batch; host copies are made on demand (view).
struct rpvg_hip_read_rows {
    uint32_t num_clusters = 0;
    uint64_t num_rows = 0, num_groups = 0, num_members = 0;
    std::vector<uint64_t> h_cluster_row_off, h_cluster_path_off;
    rpvg_hip_detail::DeviceBuffer<uint64_t> cluster_row_off, row_grp_off, grp_idx_off;
    rpvg_hip_detail::DeviceBuffer<uint32_t> row_count, path_idx;
    rpvg_hip_detail::DeviceBuffer<double> row_noise, grp_prob;
    // host copies (rpvg_hip_read_rows_view)
    bool downloaded = false;
    std::vector<uint64_t> h_row_grp_off, h_grp_idx_off;
    std::vector<uint32_t> h_row_count, h_path_idx;
    std::vector<double> h_row_noise, h_grp_prob;
    double build_ms = 0, merge_ms = 0;
};

namespace rpvg_hip_detail {

constexpr uint32_t kNone = 0xffffffffu;

// per-read padded slices: entry e of the read's (alignment, path) pairs owns slot e of every array
struct RowsScratch {
    double * align_log_prob;    // [A]
    uint32_t * surv_prefix;     // [E + N] exclusive count of survivors before an entry (slot e + read index)
    uint32_t * unit_idx;        // [E] output column of unit t (path, or name group)
    double * unit_val;          // [E] log prob, then probability of unit t
    uint32_t * tmp_idx;         // [E] (collapse) path-sorted survivors
    double * tmp_val;           // [E]
    uint32_t * bucket_of;       // [E] bucket of unit t
    double * bucket_mean;       // [E] buckets beyond the LDS capacity
    uint32_t * bucket_count;    // [E]
    uint32_t * bucket_first;    // [E] first unit (t) of bucket b
    uint32_t * bucket_rank;     // [E] position of bucket b in the sorted output
    uint32_t * bucket_cursor;   // [E]
    // outputs, padded
    double * row_noise;         // [N]
    uint32_t * row_ngroups;     // [N]
    uint32_t * row_nmembers;    // [N]
    double * grp_prob;          // [E] sorted groups of the read
    uint32_t * grp_size;        // [E]
    uint32_t * grp_moff;        // [E] exclusive member offset of the group inside the read
    uint32_t * member;          // [E]
};

// the rows of a build as the sort and merge kernels read them
struct RowView {
    const uint32_t * read_cluster;
    const uint32_t * read_count;
    const uint64_t * read_align_off;
    const uint64_t * align_path_off;
    RowsScratch sc;
    double prob_precision;
};

// The caller's sort + quickMergeIdentical (src/main.cpp:953-973) over the padded row slices (rows_merge.hip): sorts the rows of
// every cluster, finds the runs and leaves out->row_count / cluster_row_off of the merged rows; source[j] = the read whose slice
// holds merged row j.  The caller holds ctx->mutex and has set the device; waits for the stream.
int mergeRows(rpvg_hip_ctx * ctx, const rpvg_hip_alignments * al, const RowsScratch & sc, double prob_precision, rpvg_hip_read_rows * out,
              DeviceBuffer<uint32_t> * d_source, uint64_t * num_out);

}  // namespace rpvg_hip_detail

#endif

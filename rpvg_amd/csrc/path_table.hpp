// The resident path table and the name groups of an index (path_table.hip; interface include/rpvg_index.h), and what the three
// files around them — align_index.hip (the index), read_rows.hip (the rows), path_table.hip — need of one another.
#ifndef RPVG_HIP_PATH_TABLE_HPP
#define RPVG_HIP_PATH_TABLE_HPP

#include "alignments.hpp"
#include "common.hpp"

// PathInfo of every global path, device-resident (validated copy of a rpvg_path_table)
struct rpvg_hip_path_table {
    uint32_t num_paths = 0;
    uint64_t num_sources = 0;
    bool has_sources = false, has_names = false;
    rpvg_hip_detail::DeviceBuffer<uint32_t> group_id, source_count, source_id, name_id, length;
    rpvg_hip_detail::DeviceBuffer<uint64_t> source_off;
    rpvg_hip_detail::DeviceBuffer<double> effective_length;
};

// name groups of every cluster of an index and the collapsed PathInfo of every group
struct rpvg_hip_name_groups {
    uint32_t num_clusters = 0, num_paths = 0;
    uint64_t num_groups = 0;
    rpvg_hip_detail::DeviceBuffer<uint32_t> path_group;        // [P] cluster order
    rpvg_hip_detail::DeviceBuffer<uint64_t> cluster_group_off; // [K+1]
    rpvg_hip_detail::DeviceBuffer<uint32_t> group_first_path, group_name_id, group_group_id, group_source_count, group_length;  // [G]
    rpvg_hip_detail::DeviceBuffer<double> group_effective_length;                                                               // [G]
    std::vector<uint64_t> h_cluster_group_off;
    bool downloaded = false;
    std::vector<uint32_t> h_path_group, h_group_first_path, h_group_name_id, h_group_group_id, h_group_source_count, h_group_length;
    std::vector<double> h_group_effective_length;
};

namespace rpvg_hip_detail {

// what the kernels of path_table.hip read of a finished index (align_index.hip owns the arrays)
struct AlignIndexParts {
    uint32_t num_clusters = 0, num_paths = 0;
    const uint32_t * cluster_paths = nullptr;      // [P] device: global path ids in cluster order
    const uint64_t * cluster_path_off = nullptr;   // [K+1] device
    const std::vector<uint64_t> * h_cluster_path_off = nullptr;
};
bool alignIndexParts(const rpvg_hip_align_index * index, AlignIndexParts & parts);  // false: the index is not finished

// The path side of a batch whose rows are those of the index's clusters: path_group_id, the haplotype columns, h_cluster_total
// (d_row_count_u32: the rows' 32-bit read counts).  The caller holds ctx->mutex and has set the device; waits for the stream.
int attachPathSide(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch, const uint32_t * d_row_count_u32, const rpvg_hip_align_index * index,
                   const rpvg_hip_path_table * table);

}  // namespace rpvg_hip_detail

#endif

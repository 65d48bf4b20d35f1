// The device-resident alignment batch: made by rpvg_hip_alignments_upload (alignments.hip) from host arrays and by
// rpvg_hip_align_index_alignments (align_index.hip) from a finished index; read by the row kernels.
#ifndef RPVG_HIP_ALIGNMENTS_HPP
#define RPVG_HIP_ALIGNMENTS_HPP

#include "common.hpp"
#include "rows_plan.hpp"

namespace rpvg_hip_detail {
using rpvg_rows_plan::kGroupLanes;  // lanes that share a read of at most that many (alignment, path) entries (readRowSmallKernel)
}

// Device-resident alignment batch (validated copy of a rpvg_alignment_batch).
struct rpvg_hip_alignments {
    uint32_t num_clusters = 0;
    uint64_t num_reads = 0, num_aligns = 0, num_entries = 0, num_paths = 0;
    bool collapse = false;
    std::vector<uint64_t> h_cluster_read_off;  // [K+1]
    std::vector<uint64_t> h_out_path_off;      // [K+1] output columns of each cluster (paths, or name groups)
    rpvg_hip_detail::DeviceBuffer<uint32_t> read_cluster, read_count, source_count, path_group, path_idx;
    rpvg_hip_detail::DeviceBuffer<uint32_t> small_reads, large_reads;  // at most / more than 16 (alignment, path) entries
    uint64_t num_small = 0, num_large = 0;
    rpvg_hip_detail::DeviceBuffer<uint64_t> cluster_path_off, cluster_read_off, read_align_off, align_path_off;
    rpvg_hip_detail::DeviceBuffer<double> eff_len;
    rpvg_hip_detail::DeviceBuffer<uint8_t> mapq;
    rpvg_hip_detail::DeviceBuffer<int32_t> noise_score, score;
    rpvg_hip_detail::DeviceBuffer<uint16_t> align_length, frag_length;
};

#endif

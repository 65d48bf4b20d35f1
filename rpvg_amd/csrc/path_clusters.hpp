// The device part of rpvg_hip_path_clusters (path_clusters.hip) for callers whose id sets are already resident on the GPU
// (align_index.hip): a union-find over the paths, then the reference's canonical numbering.
#ifndef RPVG_HIP_PATH_CLUSTERS_HPP
#define RPVG_HIP_PATH_CLUSTERS_HPP

#include "common.hpp"

namespace rpvg_hip_detail {

struct PathClustersDevice {
    uint32_t num_paths = 0, num_clusters = 0;
    DeviceBuffer<uint32_t> parent;         // [P] union-find forest; roots after finish()
    DeviceBuffer<uint32_t> label;          // [P] path_to_cluster
    DeviceBuffer<uint32_t> path_sorted;    // [P] cluster_paths: clusters by ascending smallest path id, members ascending
    DeviceBuffer<uint64_t> cluster_off;    // [P+1] the first num_clusters + 1 are used
    DeviceBuffer<uint32_t> is_root, root_rank, path_id, label_sorted;
    DeviceBuffer<uint64_t> cluster_size;
    // allocates and makes every path its own root (num_paths > 0)
    int begin(rpvg_hip_ctx * ctx, hipStream_t st, uint32_t n);
    // joins the members of every set (device arrays; sets non-empty, ids < num_paths: the caller has checked)
    int unite(hipStream_t st, uint64_t num_sets, const uint64_t * d_set_off, const uint32_t * d_set_path);
    // flatten, number, sort; synchronises the stream and sets num_clusters
    int finish(hipStream_t st);
};

}  // namespace rpvg_hip_detail

#endif

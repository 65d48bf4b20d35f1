// What rows_text.hip reads of the resident rows where they lie: the device arrays of a rpvg_hip_read_rows (read_rows.hip), in the
// manner of table_residents.hpp.
#ifndef RPVG_HIP_ROWS_RESIDENTS_HPP
#define RPVG_HIP_ROWS_RESIDENTS_HPP

#include <cstdint>

struct rpvg_hip_read_rows;

namespace rpvg_hip_detail {

struct ReadRowsResident {
    uint32_t num_clusters;
    uint64_t num_rows, num_groups, num_members;
    const uint64_t * host_cluster_row_off;   // host [K+1]
    const uint64_t * host_cluster_path_off;  // host [K+1]
    const uint64_t * cluster_row_off;        // device [K+1]
    const uint64_t * row_grp_off;            // device [R+1]
    const uint64_t * grp_idx_off;            // device [G+1]
    const uint32_t * row_count, * path_idx;  // device [R], [M]
    const double * row_noise, * grp_prob;    // device [R], [G]
};

ReadRowsResident residentOf(const rpvg_hip_read_rows * rows);

}  // namespace rpvg_hip_detail

#endif

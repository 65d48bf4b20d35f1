// What table_text.hip reads of the two resident tables where they lie: the device arrays of a rpvg_hip_gibbs_table (gibbs_table.hip)
// and of a rpvg_hip_estimates_table (estimates_table.hip), whose structs stay private to their files.
#ifndef RPVG_HIP_TABLE_RESIDENTS_HPP
#define RPVG_HIP_TABLE_RESIDENTS_HPP

#include <cstdint>

struct rpvg_hip_gibbs_table;
struct rpvg_hip_estimates_table;

namespace rpvg_hip_detail {

struct GibbsTableResident {
    uint32_t num_clusters, num_gibbs_samples;
    uint64_t num_paths;
    const double * samples;                 // device [P * N]
    const uint8_t * listed;                 // device [P]
    const uint64_t * host_cluster_path_off; // host [K+1]
};

struct EstimatesTableResident {
    uint32_t num_clusters;
    uint64_t num_paths, num_members;
    bool has_tpm;
    const double * haplotype_prob, * read_count, * tpm;  // device [P]
    const double * member_tpm;                           // device [M]
    uint32_t ploidy;                                     // the table was built for
};

GibbsTableResident residentOf(const rpvg_hip_gibbs_table * table);
EstimatesTableResident residentOf(const rpvg_hip_estimates_table * table);

}  // namespace rpvg_hip_detail

#endif

// What both routes of the minimum path cover (path_cover.hip, path_cover_grid.hip) compute per row and per entry: one
// expression each, so that a path's weight is the same chain of the same numbers on either route.
#ifndef RPVG_HIP_COVER_TERMS_HPP
#define RPVG_HIP_COVER_TERMS_HPP

#include "common.hpp"

namespace rpvg_hip_detail {

// Utils::doubleCompare(x, 1) (src/utils.hpp:87-93)
__device__ __forceinline__ bool isOne(const double x) {
    const double precision = 2.220446049250313e-16 * 100;
    return (x == 1.0) || (fabs(x - 1.0) < fabs(fmin(x, 1.0)) * precision);
}

// the read count the cover sees: rows whose noise probability is 1 carry no reads (src/path_abundance_estimator.cpp:234-237)
__device__ __forceinline__ double coverRowCount(const double count, const double noise) { return isOne(noise) ? 0.0 : count; }

// count * log(prob), the product rounded once (:246)
__device__ __forceinline__ double coverTerm(const double prob, const double count) { return mulRounded(log(prob), count); }

// the workgroup route of the listed clusters (path_cover.hip); the caller holds the context's mutex
int minPathCoverWorkgroups(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters, const uint32_t * clusters,
                           const uint64_t * cover_off, uint32_t * cover, uint32_t * cover_size);

}  // namespace rpvg_hip_detail

#endif

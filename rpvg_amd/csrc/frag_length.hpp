// What frag_length.hip shares with read_rows.hip: the resident density table and the effective-length launch for path
// lengths that are already on the device.
#ifndef RPVG_HIP_FRAG_LENGTH_HPP
#define RPVG_HIP_FRAG_LENGTH_HPP

#include "common.hpp"

// logProb(v), v = 0 .. 65535, on the device (rpvg_hip_frag_length_table)
struct rpvg_hip_frag_table {
    double loc = 0, scale = 0, shape = 0;
    rpvg_hip_detail::DeviceBuffer<double> log_prob;  // [RPVG_FRAG_LENGTH_TABLE_SIZE]
};

namespace rpvg_hip_detail {

// effectivePathLength of d_length[0 .. n) into d_out on `stream`; the caller holds the context's lock and waits for the
// stream before `lower_scratch` (filled by the first of the two kernels) leaves scope.
int launchEffectiveLengths(hipStream_t stream, double loc, double scale, double shape, const uint32_t * d_length, uint64_t n, double * d_out,
                           DeviceBuffer<double> & lower_scratch);

}  // namespace rpvg_hip_detail

#endif

// The samples of one call of the read-count Gibbs sampler where they were drawn (gibbs_counts.hip fills the handle, gibbs_table.hip
// reads it; interface include/rpvg_samples.h): the two sample buffers in the layout of rpvg_hip_gibbs_read_counts and their two offset
// arrays, on the device and on the host.  An empty handle (no problem, or no sample) has offsets of zeros and no buffers.
#ifndef RPVG_GIBBS_SAMPLES_HPP
#define RPVG_GIBBS_SAMPLES_HPP

#include "common.hpp"

#include <vector>

struct rpvg_hip_gibbs_samples {
    uint32_t num_problems = 0;
    std::vector<uint64_t> sample_off, abund_sample_off;                             // [P+1] prefixes of num_samples and num_samples * columns
    rpvg_hip_detail::DeviceBuffer<uint64_t> d_sample_off, d_abund_sample_off;       // the same on the device
    rpvg_hip_detail::DeviceBuffer<double> d_noise_samples, d_abund_samples;         // [sample_off[P]], [abund_sample_off[P]]
};

#endif

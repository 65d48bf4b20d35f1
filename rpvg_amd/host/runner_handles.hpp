// What the harness entry points (runner_capi.cpp, tables_capi.cpp) share: the handles behind their void pointers, the one
// thread_local error string that rpvg_amd_last_error() returns, and the wrappers that turn an exception into it.  Private to the
// harness library.
#ifndef RPVG_AMD_RUNNER_HANDLES_HPP
#define RPVG_AMD_RUNNER_HANDLES_HPP

#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "estimator_factory.hpp"
#include "read_rows.hpp"

namespace rpvg_amd_harness {

using namespace rpvg_amd;

// defined once in runner_capi.cpp: one object for the whole library, read through rpvg_amd_last_error() and not exported
extern thread_local std::string last_error __attribute__((visibility("hidden")));

struct Engine {

    std::shared_ptr<HipEngine> hip;
};

// A batch resident on the GPU together with the host-side PathInfo of its clusters.
struct PreparedBatch {

    std::unique_ptr<DeviceClusterBatch> device;

    // batches that start from alignment-path lists keep the lists resident: rows can be rebuilt on the device
    std::unique_ptr<DeviceAlignmentBatch> alignments;
    std::unique_ptr<FragmentLengthDist> fragment_length_dist;
    std::unique_ptr<DeviceFragmentLengthTable> fragment_length_table;  // batches whose distribution was fitted on the device
    bool is_single_end = false;
    double min_noise_prob = 0;
    double prob_precision = 1e-8;

    std::vector<std::vector<PathInfo> > paths;

    // kept for the per-cluster estimate() mode
    std::vector<std::vector<ReadPathProbabilities> > rows;

    std::vector<PathClusterEstimates> estimates;
};

struct Result {

    std::vector<uint64_t> set_off, member_off, abund_off, em_off, em_col_off;
    std::vector<uint32_t> members, em_iters, em_cols;
    std::vector<double> posteriors, abundances, noise_count, total_count;

    std::vector<uint64_t> gibbs_off, gibbs_path_off, gibbs_noise_off, gibbs_abund_off;
    std::vector<uint32_t> gibbs_path;
    std::vector<double> gibbs_noise, gibbs_abund;
};

// f() with an exception turned into last_error and the entry point's failure value: -1 ...
template <typename F>
int guardedInt(F && f) {

    try {

        return f();

    } catch (const std::exception & e) {

        last_error = e.what();
        return -1;
    }
}

// ... or a null handle
template <typename F>
void * guardedHandle(F && f) {

    try {

        return f();

    } catch (const std::exception & e) {

        last_error = e.what();
        return nullptr;
    }
}

}

#endif

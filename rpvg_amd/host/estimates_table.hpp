// The estimates of a batch as the table rpvg writes (include/rpvg_table.h, rpvg_amd/csrc/estimates_table.hip): one row per path
// with HaplotypeProbability, ReadCount and TPM, one per group set with the members' ReadCount_i and TPM_i, and the noise of the
// `Unknown` row — instead of the three host loops over std::vector<PathClusterEstimates> (totalTranscriptCount,
// src/main.cpp:1029-1057; the writers' accumulations, src/threaded_output_writer.cpp:346-432 and :434-546).  Nothing here
// computes the table: FlatEstimates flattens the containers, EstimatesTable forwards to the GPU and holds the view; the
// writers' addTable() (io/estimates_writers.hpp) print it.
#ifndef RPVG_AMD_ESTIMATES_TABLE_HPP
#define RPVG_AMD_ESTIMATES_TABLE_HPP

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rpvg_table.h"
#include "hip_engine.hpp"
#include "path_cluster_estimates.hpp"

namespace rpvg_amd {

// The estimates of K clusters in the flat form of rpvg_estimates_flat (host memory), cluster k of the batch being entry k.
struct FlatEstimates {

    std::vector<uint64_t> set_off, member_off, abund_off, cluster_path_off;
    std::vector<uint32_t> members;
    std::vector<double> posteriors, abundances, noise_count, path_effective_length;

    FlatEstimates() : set_off(1, 0), member_off(1, 0), abund_off(1, 0), cluster_path_off(1, 0) {}

    // path_group_sets, posteriors, abundances, noise_count and the effective lengths of `paths`
    void add(const PathClusterEstimates & estimates) {

        for (size_t i = 0; i < estimates.path_group_sets.size(); ++i) {

            members.insert(members.end(), estimates.path_group_sets[i].begin(), estimates.path_group_sets[i].end());
            member_off.push_back(members.size());
            posteriors.push_back(estimates.posteriors.at(i));
        }

        set_off.push_back(posteriors.size());

        abundances.insert(abundances.end(), estimates.abundances.begin(), estimates.abundances.end());
        abund_off.push_back(abundances.size());
        noise_count.push_back(estimates.noise_count);

        for (auto & path: estimates.paths) {

            path_effective_length.push_back(path.effective_length);
        }

        cluster_path_off.push_back(path_effective_length.size());
    }

    // a copy of a host view (on_device = 0)
    static FlatEstimates copyOf(const rpvg_estimates_flat & flat) {

        FlatEstimates out;
        const size_t K = flat.num_clusters;

        if (K > 0) {

            out.set_off.assign(flat.set_off, flat.set_off + K + 1);
            out.abund_off.assign(flat.abund_off, flat.abund_off + K + 1);
            out.cluster_path_off.assign(flat.cluster_path_off, flat.cluster_path_off + K + 1);
            out.noise_count.assign(flat.noise_count, flat.noise_count + K);
            out.member_off.assign(flat.member_off, flat.member_off + flat.num_sets + 1);
        }

        if (flat.num_members) out.members.assign(flat.members, flat.members + flat.num_members);
        if (flat.num_sets) out.posteriors.assign(flat.posteriors, flat.posteriors + flat.num_sets);
        if (flat.num_abundances) out.abundances.assign(flat.abundances, flat.abundances + flat.num_abundances);
        if (flat.num_paths) out.path_effective_length.assign(flat.path_effective_length, flat.path_effective_length + flat.num_paths);

        return out;
    }

    // valid while this lives and is not added to
    rpvg_estimates_flat view() const {

        rpvg_estimates_flat flat = {};
        flat.num_clusters = noise_count.size();
        flat.num_sets = posteriors.size();
        flat.num_members = members.size();
        flat.num_abundances = abundances.size();
        flat.num_paths = path_effective_length.size();
        flat.set_off = set_off.data();
        flat.member_off = member_off.data();
        flat.members = members.data();
        flat.posteriors = posteriors.data();
        flat.abund_off = abund_off.data();
        flat.abundances = abundances.data();
        flat.noise_count = noise_count.data();
        flat.cluster_path_off = cluster_path_off.data();
        flat.path_effective_length = path_effective_length.data();
        flat.on_device = 0;

        return flat;
    }
};

// The flat estimates of a batch where the nested device calls left them: gathered on the GPU from the calls' kept blocks
// (rpvg_hip_flat_estimates_gather, rpvg_amd/csrc/estimates_gather.hip; NestedPathAbundanceEstimator::estimateBatchResident fills one).
// Owns the rpvg_hip_flat_estimates handle.  The batch it was gathered from must outlive it (cluster_path_off is the batch's array).
class ResidentEstimates {

    public:

        ResidentEstimates() : handle_(nullptr) {}
        ~ResidentEstimates() { reset(); }

        ResidentEstimates(const ResidentEstimates &) = delete;
        ResidentEstimates & operator=(const ResidentEstimates &) = delete;

        // takes the handle over (the engine's main context frees it)
        void adopt(std::shared_ptr<HipEngine> engine_in, rpvg_hip_flat_estimates * handle_in);
        void reset();

        bool empty() const { return !handle_; }
        rpvg_hip_flat_estimates * handle() const { return handle_; }

        // the device view: on_device = 1, the sizes host values
        rpvg_estimates_flat view() const;

        // host copies (one packed copy behind the first call), valid while this lives: for writers that print sets from host memory
        rpvg_estimates_flat hostView() const;
        FlatEstimates fetch() const { return FlatEstimates::copyOf(hostView()); }

        // the device memory the kept block of every lane's nested call held while the estimates were gathered (the calls'
        // capacities, not their results; the blocks are back in the pool by now): what the resident route costs in memory
        std::vector<uint64_t> kept_block_bytes;

    private:

        std::shared_ptr<HipEngine> hip_engine;
        rpvg_hip_flat_estimates * handle_;
};

class EstimatesTable {

    public:

        // from estimates resident on the GPU: built with on_device = 1, nothing is flattened or uploaded.  `resident` must outlive the table.
        EstimatesTable(std::shared_ptr<HipEngine> engine_in, const ResidentEstimates & resident_in, const uint32_t ploidy);

        // cluster k of the batch is estimates[k]; the effective lengths are those of its `paths`
        EstimatesTable(std::shared_ptr<HipEngine> engine_in, const std::vector<PathClusterEstimates> & estimates, const uint32_t ploidy);

        // a flat view in host memory (copied: the writers read it beside the table)
        EstimatesTable(std::shared_ptr<HipEngine> engine_in, const rpvg_estimates_flat & flat, const uint32_t ploidy);

        ~EstimatesTable();

        EstimatesTable(const EstimatesTable &) = delete;
        EstimatesTable & operator=(const EstimatesTable &) = delete;

        // transcript count / denominator * 1e6 for every path and member; the table's own total when the batch is the run
        void tpm(const double denominator);

        double totalTranscriptCount() { return view().total_transcript_count; }

        // host copies, fetched again when tpm() has changed the table; valid until the next tpm() or the table's end
        const rpvg_estimates_table_view & view();

        // what the table was made from (the writers print sets, posteriors and abundances from here)
        rpvg_estimates_flat estimates() const { return resident ? resident->hostView() : flat_estimates.view(); }

        // the same for a builder that reads device memory where it lies (table_text.hpp): the device view of a table made from
        // resident estimates, else the host arrays
        rpvg_estimates_flat deviceEstimates() const { return resident ? resident->view() : flat_estimates.view(); }

        // the resident table, for the builders that read it where it lies (table_text.hpp)
        rpvg_hip_estimates_table * handle() const { return table; }

    private:

        void build(const uint32_t ploidy);

        std::shared_ptr<HipEngine> hip_engine;
        FlatEstimates flat_estimates;
        const ResidentEstimates * resident = nullptr;
        rpvg_hip_estimates_table * table;
        rpvg_estimates_table_view table_view;
        bool has_view;
};

}

#endif

// The read-count Gibbs samples of a batch (-n) as the table of `<prefix>_gibbs.txt.gz` (include/rpvg_samples.h,
// rpvg_amd/csrc/gibbs_table.hip): one row of N sample columns per path in the order ReadCountGibbsSamplesWriter prints them, the rows
// it prints, and the per-sample noise totals of the `Unknown` row — instead of the per-path column vectors and the transposed read
// of ReadCountGibbsSamplesWriter::addSamples (src/threaded_output_writer.cpp:114-214).  Nothing here computes the table: FlatGibbs
// flattens the containers, GibbsSamplesTable forwards to the GPU and holds the view; the writer's addTable()
// (io/estimates_writers.hpp) prints it.
#ifndef RPVG_AMD_GIBBS_SAMPLES_TABLE_HPP
#define RPVG_AMD_GIBBS_SAMPLES_TABLE_HPP

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/rpvg_samples.h"
#include "hip_engine.hpp"
#include "io/estimates_writers.hpp"
#include "path_cluster_estimates.hpp"

namespace rpvg_amd {

// The Gibbs samples of K clusters in the flat form of rpvg_gibbs_flat (host memory), cluster k of the batch being entry k, and
// what its rows are called.
struct FlatGibbs {

    std::vector<uint64_t> gibbs_off, path_off, noise_off, abund_off, cluster_path_off;
    std::vector<uint32_t> path;
    std::vector<double> noise, abund, total_count;
    TableLabels labels;

    FlatGibbs() : gibbs_off(1, 0), path_off(1, 0), noise_off(1, 0), abund_off(1, 0), cluster_path_off(1, 0) {}

    // gibbs_read_count_samples, total_count and the names of `paths`
    void add(const uint32_t cluster_id, const PathClusterEstimates & estimates) {

        for (auto & count_samples: estimates.gibbs_read_count_samples) {

            path.insert(path.end(), count_samples.path_ids.begin(), count_samples.path_ids.end());
            path_off.push_back(path.size());
            noise.insert(noise.end(), count_samples.noise_samples.begin(), count_samples.noise_samples.end());
            noise_off.push_back(noise.size());
            abund.insert(abund.end(), count_samples.abundance_samples.begin(), count_samples.abundance_samples.end());
            abund_off.push_back(abund.size());
        }

        gibbs_off.push_back(path_off.size() - 1);
        total_count.push_back(estimates.total_count);
        labels.cluster_ids.push_back(cluster_id);

        for (auto & path_info: estimates.paths) {

            labels.names.push_back(path_info.name);
            labels.lengths.push_back(path_info.length);
        }

        cluster_path_off.push_back(labels.names.size());
    }

    // valid while this lives and is not added to
    rpvg_gibbs_flat view(const uint32_t num_gibbs_samples) const {

        rpvg_gibbs_flat flat = {};
        flat.num_clusters = total_count.size();
        flat.num_blocks = path_off.size() - 1;
        flat.num_paths = labels.names.size();
        flat.num_gibbs_samples = num_gibbs_samples;
        flat.num_path_ids = path.size();
        flat.num_noise_samples = noise.size();
        flat.num_abundance_samples = abund.size();
        flat.gibbs_off = gibbs_off.data();
        flat.gibbs_path_off = path_off.data();
        flat.gibbs_path = path.data();
        flat.gibbs_noise_off = noise_off.data();
        flat.gibbs_noise = noise.data();
        flat.gibbs_abund_off = abund_off.data();
        flat.gibbs_abund = abund.data();
        flat.cluster_path_off = cluster_path_off.data();
        flat.total_count = total_count.data();
        flat.on_device = 0;

        return flat;
    }
};

class GibbsSamplesTable {

    public:

        // cluster k of the batch is estimates_list[k].second, its ClusterID estimates_list[k].first
        GibbsSamplesTable(std::shared_ptr<HipEngine> engine_in, const ClusterEstimatesList & estimates_list, const uint32_t num_gibbs_samples_in);

        ~GibbsSamplesTable();

        GibbsSamplesTable(const GibbsSamplesTable &) = delete;
        GibbsSamplesTable & operator=(const GibbsSamplesTable &) = delete;

        // host copies of the whole table; valid until the table's end
        const rpvg_gibbs_table_view & view();

        // the sample rows of paths [first, first + count) only: count x N doubles, for a table the host could not hold twice
        std::vector<double> rows(const uint64_t first, const uint64_t count);

        // names of the rows and ClusterIDs of the clusters, for ReadCountGibbsSamplesWriter::addTable
        const TableLabels & labels() const { return flat_gibbs.labels; }

        // the resident table, for the builders that read it where it lies (table_text.hpp)
        rpvg_hip_gibbs_table * handle() const { return table; }

    private:

        std::shared_ptr<HipEngine> hip_engine;
        FlatGibbs flat_gibbs;
        const uint32_t num_gibbs_samples;
        rpvg_hip_gibbs_table * table;
        rpvg_gibbs_table_view table_view;
        bool has_view;
};

}

#endif

// The dump parsed on the GPU (rpvg_amd/csrc/rows_parse.hip) behind the host classes: ParsedDump and readProbabilityClustersDevice of
// cluster_io.hpp.  A file of its own: cluster_io.cpp stays free of the engine, so the CPU checks that compile it alone still link.
#include "cluster_io.hpp"

#include "../hip_engine.hpp"

namespace rpvg_amd {

ParsedDump::ParsedDump(const std::shared_ptr<HipEngine> & engine, const char * bytes, const uint64_t num_bytes, const bool on_device, const double prob_precision) : hip_engine(engine) {

    HipEngine::check(rpvg_hip_text_rows(hip_engine->ctx(), bytes, num_bytes, on_device ? 1 : 0, prob_precision, &dump), "rpvg_hip_text_rows");
}

ParsedDump::~ParsedDump() {

    rpvg_hip_parsed_dump_free(dump);
}

rpvg_parsed_dump_view ParsedDump::view() const {

    rpvg_parsed_dump_view out = {};
    HipEngine::check(rpvg_hip_parsed_dump_view(dump, &out), "rpvg_hip_parsed_dump_view");
    return out;
}

rpvg_cluster_batch ParsedDump::rowsView() const {

    rpvg_cluster_batch out = {};
    HipEngine::check(rpvg_hip_read_rows_view(hip_engine->ctx(), rows(), &out, nullptr, nullptr), "rpvg_hip_read_rows_view");
    return out;
}

rpvg_table_labels ParsedDump::labels() const {

    rpvg_table_labels out = {};
    HipEngine::check(rpvg_hip_parsed_dump_labels(dump, &out), "rpvg_hip_parsed_dump_labels");
    return out;
}

rpvg_hip_batch * ParsedDump::toBatch() const {

    rpvg_hip_batch * batch = nullptr;
    HipEngine::check(rpvg_hip_read_rows_to_batch(hip_engine->ctx(), rows(), &batch), "rpvg_hip_read_rows_to_batch");
    return batch;
}

std::vector<ProbabilityCluster> readProbabilityClustersDevice(const std::shared_ptr<HipEngine> & engine, const std::string & filename, const double prob_precision) {

    return readProbabilityClustersDeviceText(engine, readTextFile(filename), prob_precision);
}

std::vector<ProbabilityCluster> readProbabilityClustersDeviceText(const std::shared_ptr<HipEngine> & engine, const std::string & text, const double prob_precision) {

    const ParsedDump dump(engine, text.data(), text.size(), false, prob_precision);
    const rpvg_parsed_dump_view paths = dump.view();
    const rpvg_cluster_batch rows = dump.rowsView();

    std::vector<ProbabilityCluster> clusters(paths.num_clusters);

    for (uint32_t k = 0; k < paths.num_clusters; ++k) {

        auto & cluster = clusters[k];
        cluster.has_rank_key = paths.has_rank_key[k] != 0;
        cluster.num_align_lists = paths.num_align_lists[k];
        cluster.cluster_index = paths.cluster_index[k];

        for (uint64_t p = paths.cluster_path_off[k]; p < paths.cluster_path_off[k + 1]; ++p) {

            PathInfo path(std::string(paths.name_bytes + paths.name_off[p], paths.name_bytes + paths.name_off[p + 1]));
            path.length = paths.path_length[p];
            path.effective_length = paths.path_effective_length[p];
            cluster.paths.emplace_back(std::move(path));
        }

        for (uint64_t r = rows.cluster_row_off[k]; r < rows.cluster_row_off[k + 1]; ++r) {

            ReadPathProbabilities::PathProbs path_probs;

            for (uint64_t g = rows.row_grp_off[r]; g < rows.row_grp_off[r + 1]; ++g) {

                path_probs.emplace_back(rows.grp_prob[g], std::vector<uint32_t>(rows.path_idx + rows.grp_idx_off[g], rows.path_idx + rows.grp_idx_off[g + 1]));
            }

            cluster.cluster_probs.emplace_back(rows.row_count[r], rows.row_noise[r], path_probs, prob_precision);
        }
    }

    return clusters;
}

}

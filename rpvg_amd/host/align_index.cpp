#include "align_index.hpp"

#include <cassert>
#include <stdexcept>

#include "../../include/rpvg_hip.h"

namespace rpvg_amd {

AlignmentPathsIndex::AlignmentPathsIndex(std::shared_ptr<HipEngine> engine_in, const rpvg_index_params & params_in) : hip_engine(engine_in), params(params_in), index(nullptr), index_info(), resident_table_id(0), resident_table(nullptr), resident_groups(nullptr) {

    assert(hip_engine);
    HipEngine::check(rpvg_hip_align_index_create(hip_engine->ctx(), &params, &index), "rpvg_hip_align_index_create");
}

AlignmentPathsIndex::~AlignmentPathsIndex() {

    rpvg_hip_name_groups_free(hip_engine->ctx(), resident_groups);
    rpvg_hip_path_table_free(hip_engine->ctx(), resident_table);
    rpvg_hip_align_index_free(hip_engine->ctx(), index);
}

void AlignmentPathsIndex::add(const std::vector<std::vector<FragmentAlignmentPath> > & buffer) {

    flattenFragmentLists(buffer, &flat);
    add(flat.view());
}

void AlignmentPathsIndex::add(const rpvg_fragment_lists & chunk) {

    HipEngine::check(rpvg_hip_align_index_add(hip_engine->ctx(), index, &chunk), "rpvg_hip_align_index_add");
}

void AlignmentPathsIndex::finish(const std::vector<std::vector<uint32_t> > & extra_sets) {

    std::vector<uint64_t> set_off(1, 0);
    std::vector<uint32_t> set_path;

    for (auto & set: extra_sets) {

        set_path.insert(set_path.end(), set.begin(), set.end());
        set_off.emplace_back(set_path.size());
    }

    HipEngine::check(rpvg_hip_align_index_finish(hip_engine->ctx(), index, extra_sets.empty() ? nullptr : set_off.data(), set_path.data(), extra_sets.size(), &index_info), "rpvg_hip_align_index_finish");
}

std::vector<uint32_t> AlignmentPathsIndex::fragLengthCounts() const {

    std::vector<uint32_t> counts(static_cast<size_t>(params.max_frag_length) + 1, 0);
    HipEngine::check(rpvg_hip_align_index_frag_counts(hip_engine->ctx(), index, counts.data()), "rpvg_hip_align_index_frag_counts");

    return counts;
}

rpvg_index_view AlignmentPathsIndex::view() const {

    rpvg_index_view index_view = {};
    HipEngine::check(rpvg_hip_align_index_view(hip_engine->ctx(), index, &index_view), "rpvg_hip_align_index_view");

    return index_view;
}

std::vector<uint32_t> AlignmentPathsIndex::rankClusters() {

    const auto index_view = view();
    return std::vector<uint32_t>(index_view.rank_cluster, index_view.rank_cluster + index_view.batch.num_clusters);
}

std::vector<std::vector<uint32_t> > AlignmentPathsIndex::clusterPaths() {

    const auto index_view = view();

    std::vector<std::vector<uint32_t> > cluster_paths;
    cluster_paths.reserve(index_view.batch.num_clusters);

    for (uint32_t i = 0; i < index_view.batch.num_clusters; ++i) {

        cluster_paths.emplace_back(index_view.cluster_paths + index_view.batch.cluster_path_off[i], index_view.cluster_paths + index_view.batch.cluster_path_off[i + 1]);
    }

    return cluster_paths;
}

std::unique_ptr<DeviceAlignmentBatch> AlignmentPathsIndex::deviceAlignments(const std::vector<double> & effective_lengths) {

    if (effective_lengths.size() != params.num_paths) {

        throw std::invalid_argument("one effective length per path of the index");
    }

    rpvg_hip_alignments * alignments = nullptr;
    HipEngine::check(rpvg_hip_align_index_alignments(hip_engine->ctx(), index, effective_lengths.data(), nullptr, &alignments), "rpvg_hip_align_index_alignments");

    return std::unique_ptr<DeviceAlignmentBatch>(new DeviceAlignmentBatch(hip_engine, alignments, totalReadCounts()));
}

// the lists stay on the device; the read count of every cluster (a sum over its lists) is formed from the view's counts
std::vector<double> AlignmentPathsIndex::totalReadCounts() const {

    const auto index_view = view();
    std::vector<double> total_read_counts(index_view.batch.num_clusters, 0);

    for (uint32_t i = 0; i < index_view.batch.num_clusters; ++i) {

        uint64_t total = 0;

        for (uint64_t j = index_view.batch.cluster_read_off[i]; j < index_view.batch.cluster_read_off[i + 1]; ++j) {

            total += index_view.batch.read_count[j];
        }

        total_read_counts[i] = total;
    }

    return total_read_counts;
}

const rpvg_hip_path_table * AlignmentPathsIndex::deviceTable(const PathTable & table) const {

    if (resident_table_id != table.id() || !resident_table) {

        if (table.numPaths() != params.num_paths) {

            throw std::invalid_argument("one table entry per path of the index");
        }

        rpvg_hip_name_groups_free(hip_engine->ctx(), resident_groups);
        resident_groups = nullptr;
        rpvg_hip_path_table_free(hip_engine->ctx(), resident_table);
        resident_table = nullptr;
        resident_table_id = 0;

        const auto table_view = table.view();
        HipEngine::check(rpvg_hip_path_table_upload(hip_engine->ctx(), &table_view, &resident_table), "rpvg_hip_path_table_upload");
        resident_table_id = table.id();
    }

    return resident_table;
}

void AlignmentPathsIndex::formGroups(const PathTable & table) const {

    const auto device_table = deviceTable(table);

    if (!resident_groups) {

        HipEngine::check(rpvg_hip_align_index_name_groups(hip_engine->ctx(), index, device_table, &resident_groups), "rpvg_hip_align_index_name_groups");
    }
}

std::vector<std::vector<PathInfo> > AlignmentPathsIndex::nameGroups(const PathTable & table) const {

    formGroups(table);

    rpvg_name_groups_view groups_view = {};
    HipEngine::check(rpvg_hip_name_groups_view(hip_engine->ctx(), resident_groups, &groups_view), "rpvg_hip_name_groups_view");

    return table.collapsedPaths(groups_view);
}

std::unique_ptr<DeviceAlignmentBatch> AlignmentPathsIndex::deviceAlignmentsCollapsed(const PathTable & table) const {

    formGroups(table);

    rpvg_hip_alignments * alignments = nullptr;
    HipEngine::check(rpvg_hip_align_index_alignments_collapsed(hip_engine->ctx(), index, resident_table, resident_groups, &alignments), "rpvg_hip_align_index_alignments_collapsed");

    return std::unique_ptr<DeviceAlignmentBatch>(new DeviceAlignmentBatch(hip_engine, alignments, totalReadCounts()));
}

std::unique_ptr<DeviceAlignmentBatch> AlignmentPathsIndex::deviceAlignments(const std::vector<uint32_t> & path_lengths, const FragmentLengthDist & fragment_length_dist) {

    if (path_lengths.size() != params.num_paths) {

        throw std::invalid_argument("one path length per path of the index");
    }

    auto alignments = deviceAlignments(std::vector<double>(path_lengths.size(), 0));

    // the resident batch holds its paths in cluster order
    const auto index_view = view();
    std::vector<uint32_t> ordered_lengths(path_lengths.size());

    for (size_t i = 0; i < ordered_lengths.size(); ++i) {

        ordered_lengths[i] = path_lengths[index_view.cluster_paths[i]];
    }

    alignments->setEffectiveLengths(ordered_lengths, fragment_length_dist);

    return alignments;
}

std::unique_ptr<DeviceClusterBatch> constructReadPathProbabilities(const DeviceAlignmentBatch & alignments, const FragmentLengthDist & fragment_length_dist, const bool is_single_end, const double min_noise_prob, const double prob_precision, const AlignmentPathsIndex & index, const PathTable & table) {

    return constructReadPathProbabilities(alignments, fragment_length_dist, is_single_end, min_noise_prob, prob_precision, index.handle(), index.deviceTable(table));
}

}

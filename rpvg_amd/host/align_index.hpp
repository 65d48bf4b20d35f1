// The alignment-path index — the step between the alignment parser and row construction — behind the reference's
// shapes: what addAlignmentPathsBufferToIndexes (src/main.cpp:200-237) pops off the buffer queue goes into add(), and
// finish() leaves what the caller's cluster loop (src/main.cpp:731-754,811-827,846-905) needs: the fragment-length counts,
// the clusters in the order they are estimated in, and the distinct lists resident on the GPU as the batch
// constructReadPathProbabilities takes (include/rpvg_index.h, rpvg_amd/csrc/align_index.hip).
#ifndef RPVG_AMD_ALIGN_INDEX_HPP
#define RPVG_AMD_ALIGN_INDEX_HPP

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/rpvg_index.h"
#include "fragment_lists.hpp"
#include "hip_engine.hpp"
#include "path_table.hpp"
#include "read_rows.hpp"

namespace rpvg_amd {

class AlignmentPathsIndex {

    public:

        AlignmentPathsIndex(std::shared_ptr<HipEngine> engine_in, const rpvg_index_params & params_in);
        ~AlignmentPathsIndex();

        AlignmentPathsIndex(const AlignmentPathsIndex &) = delete;
        AlignmentPathsIndex & operator=(const AlignmentPathsIndex &) = delete;

        void add(const std::vector<std::vector<FragmentAlignmentPath> > & buffer);
        void add(const rpvg_fragment_lists & chunk);

        // extra_sets: the node-sharing sets of PathClusters::addNodeClusters
        void finish(const std::vector<std::vector<uint32_t> > & extra_sets = std::vector<std::vector<uint32_t> >());

        const rpvg_index_info & info() const { return index_info; }
        uint64_t numDistinct() const { return index_info.num_distinct; }

        // frag_length_counts of src/main.cpp:203-216, for FragmentLengthDist(counts, skew_normal)
        std::vector<uint32_t> fragLengthCounts() const;

        // the PathClusters index of the cluster estimated first, second, ... (src/main.cpp:811-827)
        std::vector<uint32_t> rankClusters();

        // the global path ids of every cluster in that order, ascending (path_clusters.cluster_to_paths_index)
        std::vector<std::vector<uint32_t> > clusterPaths();

        // The distinct lists as the resident batch of row construction.  effective_lengths / path_lengths: one per GLOBAL path.
        std::unique_ptr<DeviceAlignmentBatch> deviceAlignments(const std::vector<double> & effective_lengths);
        std::unique_ptr<DeviceAlignmentBatch> deviceAlignments(const std::vector<uint32_t> & path_lengths, const FragmentLengthDist & fragment_length_dist);

        // `-i transcripts --path-info` (collapse_haps): the name groups of every cluster and their collapsed paths, formed on
        // the GPU (group_name_index, src/main.cpp:853-887, and :909-951); every name is that of its group's first member.  The
        // table stays resident in the index until one with other contents (PathTable::id) is handed in.
        std::vector<std::vector<PathInfo> > nameGroups(const PathTable & table) const;

        // The distinct lists as the resident batch of row construction with the groups of nameGroups(table) as its output
        // columns (source counts and effective lengths from the table).
        std::unique_ptr<DeviceAlignmentBatch> deviceAlignmentsCollapsed(const PathTable & table) const;

        // what constructReadPathProbabilities (below) hands to rpvg_hip_read_rows_to_batch_with_paths
        const rpvg_hip_align_index * handle() const { return index; }
        const rpvg_hip_path_table * deviceTable(const PathTable & table) const;

    private:

        rpvg_index_view view() const;
        std::vector<double> totalReadCounts() const;
        void formGroups(const PathTable & table) const;

        std::shared_ptr<HipEngine> hip_engine;
        rpvg_index_params params;
        rpvg_hip_align_index * index;
        rpvg_index_info index_info;
        FlatFragmentLists flat;

        // the table last handed in, resident, and its groups: a cache that does not change what the index is
        mutable uint64_t resident_table_id;
        mutable rpvg_hip_path_table * resident_table;
        mutable rpvg_hip_name_groups * resident_groups;
};

// The rows of `alignments` (made by index.deviceAlignments) as the batch the estimators take, with its path side — group ids,
// haplotype columns (DeviceClusterBatch::hasSourceColumns), read totals — formed on the GPU from the table.
std::unique_ptr<DeviceClusterBatch> constructReadPathProbabilities(const DeviceAlignmentBatch & alignments, const FragmentLengthDist & fragment_length_dist, const bool is_single_end, const double min_noise_prob, const double prob_precision, const AlignmentPathsIndex & index, const PathTable & table);

}

#endif

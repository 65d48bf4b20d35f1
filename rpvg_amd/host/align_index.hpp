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

    private:

        rpvg_index_view view();

        std::shared_ptr<HipEngine> hip_engine;
        rpvg_index_params params;
        rpvg_hip_align_index * index;
        rpvg_index_info index_info;
        FlatFragmentLists flat;
};

}

#endif

// The per-fragment alignment-path lists of the alignment-path index (align_index.hpp) and their flat layout
// (include/rpvg_index.h).  Plain host code: no engine, no device.
#ifndef RPVG_AMD_FRAGMENT_LISTS_HPP
#define RPVG_AMD_FRAGMENT_LISTS_HPP

#include <cstdint>
#include <vector>

#include "../../include/rpvg_index.h"

namespace rpvg_amd {

// The AlignmentPath of the reference at the fragment level (src/alignment_path.hpp:22-39): the fields that take part in
// the index, the gbwt search state replaced by the GLOBAL ids of the paths it locates (ascending).  The last entry of a
// list is the noise entry: no paths.  (AlignmentPath of read_rows.hpp is the cluster-local form row construction reads.)
struct FragmentAlignmentPath {

    bool is_simple = false;
    uint8_t min_mapq = 0;
    int32_t score_sum = 0;
    uint16_t align_length = 0;
    uint16_t frag_length = 0;

    std::vector<uint32_t> path_ids;

    FragmentAlignmentPath() {}
    FragmentAlignmentPath(const bool is_simple_in, const uint8_t min_mapq_in, const int32_t score_sum_in, const uint16_t align_length_in, const uint16_t frag_length_in, const std::vector<uint32_t> & path_ids_in) : is_simple(is_simple_in), min_mapq(min_mapq_in), score_sum(score_sum_in), align_length(align_length_in), frag_length(frag_length_in), path_ids(path_ids_in) {}
};

// One buffer of lists in the flat layout of rpvg_fragment_lists.
struct FlatFragmentLists {

    std::vector<uint8_t> list_is_simple, list_min_mapq;
    std::vector<int32_t> list_noise_score, align_score_sum;
    std::vector<uint64_t> list_align_off, align_path_off;
    std::vector<uint16_t> align_length, align_frag_length;
    std::vector<uint32_t> align_path_id;

    rpvg_fragment_lists view() const;
};

// The loop body of the queue's consumer without a device: every list's front gives is_simple and min_mapq, its back (the
// noise entry) the noise score, the entries in between the alignments.  Throws std::invalid_argument for an empty list;
// everything else (a list of the noise entry alone, an alignment without paths, ...) is left for the device to refuse.
void flattenFragmentLists(const std::vector<std::vector<FragmentAlignmentPath> > & buffer, FlatFragmentLists * flat);

}

#endif

#include "fragment_lists.hpp"

#include <cassert>
#include <stdexcept>

namespace rpvg_amd {

rpvg_fragment_lists FlatFragmentLists::view() const {

    rpvg_fragment_lists chunk = {};
    chunk.num_lists = list_is_simple.size();
    chunk.list_is_simple = list_is_simple.data();
    chunk.list_min_mapq = list_min_mapq.data();
    chunk.list_noise_score = list_noise_score.data();
    chunk.list_align_off = list_align_off.data();
    chunk.align_score_sum = align_score_sum.data();
    chunk.align_length = align_length.data();
    chunk.align_frag_length = align_frag_length.data();
    chunk.align_path_off = align_path_off.data();
    chunk.align_path_id = align_path_id.data();

    return chunk;
}

void flattenFragmentLists(const std::vector<std::vector<FragmentAlignmentPath> > & buffer, FlatFragmentLists * flat) {

    assert(flat);

    flat->list_is_simple.clear();
    flat->list_min_mapq.clear();
    flat->list_noise_score.clear();
    flat->align_score_sum.clear();
    flat->align_length.clear();
    flat->align_frag_length.clear();
    flat->align_path_id.clear();

    flat->list_align_off.assign(1, 0);
    flat->align_path_off.assign(1, 0);

    flat->list_is_simple.reserve(buffer.size());
    flat->list_min_mapq.reserve(buffer.size());
    flat->list_noise_score.reserve(buffer.size());
    flat->list_align_off.reserve(buffer.size() + 1);

    for (auto & align_paths: buffer) {

        if (align_paths.empty()) {

            throw std::invalid_argument("an alignment-path list holds its noise entry at least");
        }

        flat->list_is_simple.emplace_back(align_paths.front().is_simple ? 1 : 0);
        flat->list_min_mapq.emplace_back(align_paths.front().min_mapq);
        flat->list_noise_score.emplace_back(align_paths.back().score_sum);

        for (size_t i = 0; i + 1 < align_paths.size(); ++i) {

            const auto & align_path = align_paths[i];

            flat->align_score_sum.emplace_back(align_path.score_sum);
            flat->align_length.emplace_back(align_path.align_length);
            flat->align_frag_length.emplace_back(align_path.frag_length);
            flat->align_path_id.insert(flat->align_path_id.end(), align_path.path_ids.begin(), align_path.path_ids.end());
            flat->align_path_off.emplace_back(flat->align_path_id.size());
        }

        flat->list_align_off.emplace_back(flat->align_score_sum.size());
    }
}

}

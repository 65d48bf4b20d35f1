// The host flattening of AlignmentPathsIndex::add (rpvg_amd/host/fragment_lists.hpp) without a device: buffers of alignment-path
// lists as addAlignmentPathsToBuffer emits them -> the flat layout of include/rpvg_index.h.  Stand-alone; built with
// -fsanitize=address,undefined by tests/test_align_index_model.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "fragment_lists.hpp"

using rpvg_amd::FlatFragmentLists;
using rpvg_amd::FragmentAlignmentPath;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static FragmentAlignmentPath noise(const int32_t score) { return FragmentAlignmentPath(false, 0, score, 0, 0, {}); }

// the flat chunk read back list by list
static void checkRoundTrip(const std::vector<std::vector<FragmentAlignmentPath> > & buffer, const FlatFragmentLists & flat) {

    const rpvg_fragment_lists chunk = flat.view();
    CHECK(chunk.num_lists == buffer.size());
    CHECK(flat.list_align_off.size() == buffer.size() + 1 && flat.list_align_off.front() == 0);
    CHECK(flat.align_path_off.size() == flat.align_score_sum.size() + 1 && flat.align_path_off.front() == 0);
    CHECK(flat.align_path_off.back() == flat.align_path_id.size());
    CHECK(flat.list_align_off.back() == flat.align_score_sum.size());
    CHECK(flat.align_length.size() == flat.align_score_sum.size() && flat.align_frag_length.size() == flat.align_score_sum.size());

    for (size_t i = 0; i < buffer.size(); ++i) {

        const auto & list = buffer[i];
        CHECK(chunk.list_is_simple[i] == (list.front().is_simple ? 1 : 0));
        CHECK(chunk.list_min_mapq[i] == list.front().min_mapq);
        CHECK(chunk.list_noise_score[i] == list.back().score_sum);
        CHECK(chunk.list_align_off[i + 1] - chunk.list_align_off[i] == list.size() - 1);

        for (size_t j = 0; j + 1 < list.size(); ++j) {

            const uint64_t a = chunk.list_align_off[i] + j;
            CHECK(chunk.align_score_sum[a] == list[j].score_sum);
            CHECK(chunk.align_length[a] == list[j].align_length);
            CHECK(chunk.align_frag_length[a] == list[j].frag_length);
            CHECK(chunk.align_path_off[a + 1] - chunk.align_path_off[a] == list[j].path_ids.size());

            for (size_t k = 0; k < list[j].path_ids.size(); ++k) {

                CHECK(chunk.align_path_id[chunk.align_path_off[a] + k] == list[j].path_ids[k]);
            }
        }
    }
}

int main() {

    FlatFragmentLists flat;

    // an empty buffer: one offset each, nothing else
    rpvg_amd::flattenFragmentLists({}, &flat);
    CHECK(flat.view().num_lists == 0 && flat.list_align_off.size() == 1 && flat.align_path_off.size() == 1);

    // the case of tests/align_index_model.py, hand_case(): six lists, the noise entry last
    std::vector<std::vector<FragmentAlignmentPath> > buffer = {
        {FragmentAlignmentPath(true, 40, 10, 50, 7, {4, 5}), noise(-3)},
        {FragmentAlignmentPath(true, 29, 8, 40, 6, {0}), FragmentAlignmentPath(true, 29, 7, 40, 6, {1}), noise(-3)},
        {FragmentAlignmentPath(true, 40, 12, 60, 9, {4, 5}), noise(-3)},
        {FragmentAlignmentPath(false, 40, 10, 50, 7, {4, 5}), noise(-3)},
        {FragmentAlignmentPath(true, 60, 5, 30, 10, {2}), noise(0)},
        {FragmentAlignmentPath(true, 29, 8, 40, 6, {0}), FragmentAlignmentPath(true, 29, 7, 40, 6, {1}), noise(-3)}};
    rpvg_amd::flattenFragmentLists(buffer, &flat);
    checkRoundTrip(buffer, flat);
    CHECK((flat.list_align_off == std::vector<uint64_t>{0, 1, 3, 4, 5, 6, 8}));
    CHECK((flat.align_path_off == std::vector<uint64_t>{0, 2, 3, 4, 6, 8, 9, 10, 11}));
    CHECK((flat.align_path_id == std::vector<uint32_t>{4, 5, 0, 1, 4, 5, 4, 5, 2, 0, 1}));
    CHECK((flat.list_noise_score == std::vector<int32_t>{-3, -3, -3, -3, 0, -3}));
    CHECK((flat.list_is_simple == std::vector<uint8_t>{1, 1, 1, 0, 1, 1}));

    // the same object is reused from buffer to buffer (AlignmentPathsIndex::add): a shorter buffer leaves nothing behind
    buffer.resize(2);
    rpvg_amd::flattenFragmentLists(buffer, &flat);
    checkRoundTrip(buffer, flat);
    CHECK(flat.align_path_id.size() == 4);

    // a list of its noise entry alone and an alignment without paths are passed on as they are (the device refuses them)
    buffer = {{noise(-1)}, {FragmentAlignmentPath(true, 1, 2, 3, 4, {}), noise(-2)}};
    rpvg_amd::flattenFragmentLists(buffer, &flat);
    checkRoundTrip(buffer, flat);
    CHECK((flat.list_align_off == std::vector<uint64_t>{0, 0, 1}) && (flat.align_path_off == std::vector<uint64_t>{0, 0}));

    // an empty list has no front or back to read
    bool thrown = false;
    try {
        rpvg_amd::flattenFragmentLists({{}}, &flat);
    } catch (const std::invalid_argument &) {
        thrown = true;
    }
    CHECK(thrown);

    // random buffers, long lists included
    std::mt19937 rng(7);
    for (int round = 0; round < 50; ++round) {

        buffer.clear();
        const int num_lists = rng() % 200;

        for (int i = 0; i < num_lists; ++i) {

            buffer.emplace_back();
            const int num_aligns = (rng() % 20 == 0) ? 30 : 1 + rng() % 4;

            for (int j = 0; j < num_aligns; ++j) {

                std::vector<uint32_t> ids;
                uint32_t id = rng() % 50;

                for (int k = 1 + rng() % 6; k > 0; --k) {

                    ids.push_back(id);
                    id += 1 + rng() % 9;
                }

                buffer.back().emplace_back(rng() % 2, rng() % 61, static_cast<int32_t>(rng() % 300), rng() % 65536, rng() % 65536, ids);
            }

            buffer.back().emplace_back(noise(-static_cast<int32_t>(rng() % 100)));
        }

        rpvg_amd::flattenFragmentLists(buffer, &flat);
        checkRoundTrip(buffer, flat);
    }

    std::printf("ok\n");
    return 0;
}

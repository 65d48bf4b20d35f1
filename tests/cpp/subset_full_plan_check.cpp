// The host-side arithmetic of rpvg_hip_nested_full_subset_em (rpvg_amd/csrc/subset_full_plan.hpp) on the CPU: the map from a set's
// rank to its members against explicit enumeration, the slots of a matrix, the cuts of a batch into launches either side of 2^27
// sets, every refusal that needs no device, and the packed layout.  A program of its own, built with the sanitizers:
//   g++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -I rpvg_amd/csrc tests/cpp/subset_full_plan_check.cpp
#include "subset_full_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rpvg_subset_full;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static bool sameMembers(const uint32_t * a, const std::vector<uint32_t> & b) {
    for (size_t i = 0; i < b.size(); ++i) {
        if (a[i] != b[i]) return false;
    }
    return true;
}

int main() {
    // unranking against the odometer of PathClusterEstimates::generateGroups: rank 0, the last rank and every 97th in between
    for (uint32_t g = 1; g <= 8; ++g) {
        for (uint32_t G = 1; G <= 12; ++G) {
            const uint64_t sets = setCount(G, g);
            std::vector<uint32_t> set(g, 0);
            uint64_t rank = 0;
            for (;; ++rank) {
                if (rank == 0 || rank + 1 == sets || rank % 97 == 0) {
                    uint32_t members[8] = {9, 9, 9, 9, 9, 9, 9, 9};
                    unrankSet(G, g, rank, members);
                    CHECK(sameMembers(members, set));
                    CHECK(rankOfSet(G, g, members) == rank);
                }
                int k = static_cast<int>(g) - 1;
                while (k >= 0 && set[k] + 1 == G) --k;
                if (k < 0) break;
                const uint32_t v = set[k] + 1;
                for (uint32_t j = k; j < g; ++j) set[j] = v;
            }
            CHECK(rank + 1 == sets);
        }
    }
    // the last rank of a problem at the bound (RPVG_HIP_FULL_MAX_SETS): the widest problem the bound admits at every group size
    for (uint32_t g = 1; g <= 8; ++g) {
        uint32_t G = 1;
        if (g == 1) {
            G = static_cast<uint32_t>(kMaxSets);
        } else {
            while (setCount(G + 1, g) <= kMaxSets) ++G;
        }
        const uint64_t sets = setCount(G, g);
        CHECK(sets <= kMaxSets && setCount(G + 1, g) > kMaxSets);
        if (g == 1) CHECK(sets == kMaxSets);
        uint32_t members[8];
        unrankSet(G, g, sets - 1, members);
        for (uint32_t i = 0; i < g; ++i) CHECK(members[i] == G - 1);
        CHECK(rankOfSet(G, g, members) == sets - 1);
        unrankSet(G, g, 0, members);
        for (uint32_t i = 0; i < g; ++i) CHECK(members[i] == 0);
        if (g > 1) {  // the set behind the first carry: (0, .., 0, 1, 1) follows (0, .., 0, G - 1)
            unrankSet(G, g, G, members);
            CHECK(members[g - 1] == 1 && members[g - 2] == 1);
        }
    }
    CHECK(setCount(0, 3) == 0 && setCount(5, 0) == 1 && setCount(30, 6) == 1623160 && setCount(200, 8) > kMaxSets);
    CHECK(setCount(4000000000u, 8) == UINT64_MAX);

    // slots
    CHECK(slotsOf(0) == 0 && slotsOf(1) == 1 && slotsOf(1023) == 1023 && slotsOf(1024) == 1024 && slotsOf(1025) == 1024 && slotsOf(kMaxSets) == 1024);

    // launches: up to 2^27 sets, a larger problem alone, a problem never split
    {
        const uint64_t cut = kSetsPerLaunch;
        const uint64_t a[] = {cut - 1, 1, 1};
        CHECK(chunkEnd(a, 0, 3) == 2 && chunkEnd(a, 2, 3) == 3);
        const uint64_t b[] = {cut, 1};
        CHECK(chunkEnd(b, 0, 2) == 1 && chunkEnd(b, 1, 2) == 2);
        const uint64_t c[] = {cut + 1, 1};
        CHECK(chunkEnd(c, 0, 2) == 1);
        const uint64_t d[] = {1, cut + 1, 1};
        CHECK(chunkEnd(d, 0, 3) == 1 && chunkEnd(d, 1, 3) == 2 && chunkEnd(d, 2, 3) == 3);
        const uint64_t e[] = {1, cut - 1, 1};
        CHECK(chunkEnd(e, 0, 3) == 2);
        const uint64_t f[] = {76904685, 76904685};  // two problems of group size 8 over 33 columns: together past the cut
        CHECK(setCount(33, 8) == 76904685 && chunkEnd(f, 0, 2) == 1 && chunkEnd(f, 1, 2) == 2);
        const uint64_t z[] = {0, 0, 5};
        CHECK(chunkEnd(z, 0, 3) == 3 && chunkEnd(z, 0, 0) == 0);
    }

    // refusals
    {
        const uint32_t columns[] = {4, 30, 1};
        CallShape ok;
        ok.group_size = 6;
        ok.min_hap_prob = 1e-3;
        ok.num_matrices = 3;
        ok.columns = columns;
        ok.max_paths = 100;
        ok.has_group_ids = true;
        uint32_t which = 77;
        CHECK(refusal(ok, &which) == kTaken && which == 77);
        for (uint32_t g = 0; g <= 10; ++g) {
            CallShape c = ok;
            c.group_size = g;
            CHECK((refusal(c, nullptr) == kGroupSize) == (g == 0 || g == 2 || g > 8));
        }
        CallShape c = ok;
        c.min_hap_prob = 1.0 / 1024;
        CHECK(refusal(c, nullptr) == kTaken);
        c.min_hap_prob = 1.0 / 2048;
        CHECK(refusal(c, nullptr) == kMinHapProb);
        c.min_hap_prob = 0.0;
        CHECK(refusal(c, nullptr) == kMinHapProb);
        c = ok;
        c.has_group_ids = false;
        CHECK(refusal(c, nullptr) == kNoGroupIds);
        c = ok;
        c.disabled = true;
        CHECK(refusal(c, nullptr) == kDisabled);
        const uint32_t wide[] = {4, 200, 300};
        c = ok;
        c.group_size = 8;
        c.columns = wide;
        CHECK(refusal(c, &which) == kTooManySets && which == 1);
        c = ok;
        c.max_paths = 3991;  // (the diploid call's rule: 8 (5 (paths + 1) + 6) bytes against 156 KiB)
        CHECK(emVectorsFit(3991) && !emVectorsFit(3993) && refusal(c, nullptr) == kTaken);
        c.max_paths = 3993;
        CHECK(refusal(c, nullptr) == kTooWide);
        c.num_matrices = 0;
        CHECK(refusal(c, nullptr) == kTaken);
    }

    // the packed layout: group size 0 is the diploid call's (two members per set slot); every array 64-byte aligned and apart
    {
        const PackedLayout d = packedLayout(3, 5, 17, 11);
        CHECK(d.subset_off == 0 && d.weight == 64 && d.path_off == 128 && d.set_abund - d.set_posterior == 192 && d.merge_flags - d.set_abund == 320);
        CHECK(d.bytes == d.merge_flags + 64);
        for (uint32_t g = 1; g <= 8; ++g) {
            const PackedLayout p = packedLayout(3, 5, 17, 11, g, 9);
            const size_t at[] = {p.subset_off, p.weight, p.path_off, p.col_off, p.abundances, p.noise, p.total, p.path, p.col_path, p.iterations,
                                 p.kept_rows, p.kept_entries, p.set_count, p.cluster_noise, p.set_posterior, p.set_abund, p.merge_flags, p.set_size,
                                 p.set_member, p.retained_off, p.retained_rank, p.retained_posterior, p.bytes};
            const size_t need[] = {32, 40, 48, 48, 88, 40, 40, 68, 44, 20, 20, 20, 12, 24, 136, 136ul * g, 64, 68, 68ul * g, 32, 72, 72};
            for (size_t i = 0; i + 1 < sizeof(at) / sizeof(at[0]); ++i) {
                CHECK(at[i] % 64 == 0 && at[i] + need[i] <= at[i + 1]);
            }
            CHECK(p.subset_off == d.subset_off && p.cluster_noise == d.cluster_noise);
        }
    }
    std::printf("ok\n");
    return 0;
}

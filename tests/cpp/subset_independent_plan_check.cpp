// The host-side plan of rpvg_hip_nested_independent_subset_em (rpvg_amd/csrc/subset_independent_plan.hpp) on the CPU: the number
// of samples, the weight table against a literal loop, word counts and capacities either side of a 624-word block, every refusal.
// Built by tests/test_independent_model.py with AddressSanitizer and UBSan; prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "subset_independent_plan.hpp"

using namespace rpvg_subset_independent;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

int main() {
    // S = floor(1 / min_hap_prob) in double
    CHECK(numSamples(0.5) == 2);
    CHECK(numSamples(1.0 / 312) == 312);
    CHECK(numSamples(1.0 / 313) == static_cast<uint32_t>(std::floor(1 / (1.0 / 313))));
    CHECK(numSamples(1.0 / 313) == 313);
    CHECK(numSamples(0.001) == 1000);
    CHECK(numSamples(1.0 / 1024) == 1024);
    CHECK(numSamples(1.0) == 1);
    CHECK(numSamples(0.0) == 0 && numSamples(-1.0) == 0 && numSamples(1.5) == 0 && numSamples(std::nan("")) == 0);

    // the weight table: a chain of additions, not count / S
    for (const double p: {0.5, 1.0 / 312, 1.0 / 313, 0.001, 1.0 / 1024}) {
        const uint32_t S = numSamples(p);
        std::vector<double> table(S + 1);
        weightTable(S, table.data());
        double w = 0.0;
        CHECK(table[0] == 0.0);
        for (uint32_t c = 1; c <= S; ++c) {
            w += 1 / static_cast<double>(S);
            CHECK(table[c] == w);
        }
        CHECK(table[1] >= p);  // 1 / floor(1 / p) >= p: one sample is enough to be retained
    }
    {
        std::vector<double> table(1001);
        weightTable(1000, table.data());
        CHECK(table[1000] == 1.0000000000000007);
        CHECK(table[1000] != 1000 / 1000.0);
        CHECK(table[3] != 3 / 1000.0 || table[7] != 7 / 1000.0 || table[1000] != 1.0);
    }

    // words and blocks either side of a block of 624 words
    CHECK(wordsConsumed(2, 0) == 0 && streamBlocks(0) == 0 && !stateReturned(0));
    CHECK(wordsConsumed(2, 1) == 4 && streamBlocks(4) == 1 && !stateReturned(4));
    CHECK(wordsConsumed(312, 1) == 624 && streamBlocks(624) == 1 && stateReturned(624));
    CHECK(wordsConsumed(313, 1) == 626 && streamBlocks(626) == 2 && stateReturned(626));
    CHECK(wordsConsumed(311, 1) == 622 && streamBlocks(622) == 1 && !stateReturned(622));
    CHECK(wordsConsumed(312, 3) == 1872 && streamBlocks(1872) == 3);
    CHECK(wordsConsumed(313, 3) == 1878 && streamBlocks(1878) == 4);
    CHECK(wordsConsumed(1024, 4000000) == 8192000000ull);  // no 32-bit overflow
    {
        const ClusterCapacity c = clusterCapacity(1000, 7, 2);
        CHECK(c.samples == 1000 && c.subsets == 1000 && c.path_slots == 14000 && c.words_bound == 14000);
        const ClusterCapacity none = clusterCapacity(2, 0, 8);
        CHECK(none.path_slots == 0 && none.words_bound == 0);
    }

    // refusals
    {
        const uint32_t columns[3] = {2, 5, 1};
        CallShape shape;
        shape.group_size = 2;
        shape.min_hap_prob = 0.001;
        shape.num_matrices = 3;
        shape.columns = columns;
        shape.max_paths = 8;
        shape.has_group_ids = true;
        uint32_t which = 99;
        CHECK(refusal(shape, &which) == kTaken);
        for (uint32_t g = 1; g <= 8; ++g) {
            CallShape s = shape;
            s.group_size = g;
            CHECK(refusal(s, &which) == kTaken);
        }
        CallShape s = shape;
        s.group_size = 0;
        CHECK(refusal(s, &which) == kGroupSize);
        s.group_size = 9;
        CHECK(refusal(s, &which) == kGroupSize);
        s = shape;
        s.disabled = true;
        CHECK(refusal(s, &which) == kDisabled);
        s = shape;
        s.min_hap_prob = 1.0 / 1025;
        CHECK(refusal(s, &which) == kMinHapProb);
        s.min_hap_prob = 1.0 / 1024;
        CHECK(refusal(s, &which) == kTaken);
        s.min_hap_prob = 1.0;
        CHECK(refusal(s, &which) == kTaken);
        s.min_hap_prob = 1.0000001;
        CHECK(refusal(s, &which) == kMinHapProb);
        s.min_hap_prob = std::nan("");
        CHECK(refusal(s, &which) == kMinHapProb);
        s = shape;
        s.has_group_ids = false;
        CHECK(refusal(s, &which) == kNoGroupIds);
        {
            const uint32_t with_empty[3] = {2, 0, 1};
            s = shape;
            s.columns = with_empty;
            CHECK(refusal(s, &which) == kNoSet && which == 1);
        }
        {
            // 361 columns have 65 341 pairs, 362 have 65 703
            const uint32_t wide[3] = {2, 361, 362};
            s = shape;
            s.columns = wide;
            CHECK(refusal(s, &which) == kTooManySets && which == 2);
            const uint32_t fits[3] = {2, 361, 361};
            s.columns = fits;
            CHECK(refusal(s, &which) == kTaken);
            s.group_size = 1;
            const uint32_t singles[3] = {65536, 65537, 1};
            s.columns = singles;
            CHECK(refusal(s, &which) == kTooManySets && which == 1);
        }
        s = shape;
        s.max_paths = 4000;
        CHECK(rpvg_subset_full::emVectorsFit(3000) && !rpvg_subset_full::emVectorsFit(4000));
        CHECK(refusal(s, &which) == kTooWide);
        s = shape;
        s.num_matrices = 3000000;  // 1 000 samples x 3 M transcripts x 12 bytes
        std::vector<uint32_t> many(s.num_matrices, 1);
        s.columns = many.data();
        CHECK(refusal(s, &which) == kCapacity);
        for (const Refusal r: {kGroupSize, kDisabled, kMinHapProb, kNoGroupIds, kNoSet, kTooManySets, kTooWide, kCapacity}) {
            CHECK(refusalText(r)[0] != 0);
        }
    }
    std::printf("ok\n");
    return 0;
}

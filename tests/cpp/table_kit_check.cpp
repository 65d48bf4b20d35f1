// The pure part of rpvg_amd/csrc/table_kit.hpp on the CPU: the offender word (encode, decode, its order), lastAtMost and offsetsBad.
// Built by g++ against table_kit.hpp alone (tests/test_table_kit.py); prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "table_kit.hpp"

using namespace rpvg_hip_detail;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

namespace {

// the largest reason in use: kBadPathOrder of gibbs_table.hip (estimates 6, align_index 5, path_table 3)
constexpr int kMaxWhyInUse = 9;
constexpr uint64_t kIndices[] = {0, 1, 0x7fffffffull};  // the largest index a table admits: 2^31 - 1

void offenderWordChecks() {
    static_assert(kMaxWhyInUse < static_cast<int>(kWhyRadix), "every reason in use fits the radix");
    for (const bool second : {false, true}) {
        for (const uint64_t index : kIndices) {
            for (int why = 1; why <= kMaxWhyInUse; ++why) {
                const word64 word = offenderWord(index, why, second);
                CHECK(word != kNoBad);
                const Offender o = offenderOf(word, kMaxWhyInUse);
                CHECK(o.second_kind == second && o.index == index && o.why == why);
                // a reason beyond what the caller knows decodes to 0; kind and index stay
                const Offender narrow = offenderOf(word, why - 1);
                CHECK(narrow.why == 0 && narrow.index == index && narrow.second_kind == second);
            }
            for (int why = kMaxWhyInUse + 1; why < static_cast<int>(kWhyRadix); ++why) {
                CHECK(offenderOf(offenderWord(index, why, second), kMaxWhyInUse).why == 0);
            }
        }
    }
    // the minimum of two words of one kind: the smaller index, at equal index the smaller reason
    for (const bool second : {false, true}) {
        for (const uint64_t i : kIndices) {
            for (const uint64_t j : kIndices) {
                for (int a = 1; a <= kMaxWhyInUse; ++a) {
                    for (int b = 1; b <= kMaxWhyInUse; ++b) {
                        const word64 x = offenderWord(i, a, second), y = offenderWord(j, b, second);
                        const Offender least = offenderOf(x < y ? x : y, kMaxWhyInUse);
                        if (i != j) CHECK(least.index == (i < j ? i : j) && least.why == (i < j ? a : b));
                        else CHECK(least.index == i && least.why == (a < b ? a : b));
                    }
                }
            }
        }
    }
    // every word of the first kind (a cluster) is below every word of the second (a block)
    for (const uint64_t i : kIndices) {
        for (const uint64_t j : kIndices) {
            for (int a = 1; a < static_cast<int>(kWhyRadix); ++a) {
                for (int b = 1; b < static_cast<int>(kWhyRadix); ++b) CHECK(offenderWord(i, a, false) < offenderWord(j, b, true));
            }
        }
    }
}

uint64_t linearLastAtMost(const std::vector<uint64_t> & off, const uint64_t x) {
    uint64_t last = 0;
    for (uint64_t i = 0; i < off.size(); ++i) {
        if (off[i] <= x) last = i;
    }
    return last;
}

void lastAtMostChecks() {
    std::mt19937_64 rng(7);
    for (const uint64_t n : {1ull, 2ull, 3ull, 64ull, 65ull}) {
        std::vector<uint64_t> ascending(n), constant(n, 5), descending(n), random(n);
        for (uint64_t i = 0; i < n; ++i) {
            ascending[i] = 3 * i;  // from 0, as offsets do
            descending[i] = 3 * (n - i);
            random[i] = rng();
        }
        std::vector<uint64_t> probes = {0, 1, 2, 3, 4, 5, 6, 3 * n - 1, 3 * n, 3 * n + 1, ~0ull};
        for (uint64_t i = 0; i < n; ++i) {
            probes.push_back(3 * i);
            probes.push_back(3 * i + 1);
            probes.push_back(random[i]);
        }
        for (const uint64_t x : probes) {
            CHECK(lastAtMost(ascending.data(), n, x) == linearLastAtMost(ascending, x));
            for (const auto * contents : {&ascending, &constant, &descending, &random}) CHECK(lastAtMost(contents->data(), n, x) < n);
        }
    }
}

void offsetsBadChecks() {
    std::mt19937_64 rng(11);
    for (int round = 0; round < 20000; ++round) {
        const uint64_t n = 1 + rng() % 4, total = rng() % 6;
        std::vector<uint64_t> off(n + 1);
        for (auto & o : off) o = rng() % 7;
        if (round % 3 == 0) {  // a valid array now and then
            off[0] = 0;
            for (uint64_t i = 1; i <= n; ++i) off[i] = off[i - 1] + (i == n ? total - off[i - 1] : rng() % (total - off[i - 1] + 1));
        }
        for (uint64_t i = 0; i < n; ++i) {
            const bool literal = off[i] > off[i + 1] || off[i + 1] > total || (i == 0 && off[i] != 0) || (i + 1 == n && off[i + 1] != total);
            CHECK(offsetsBad(off.data(), i, n, total) == literal);
            if (round % 3 == 0) CHECK(!literal);
        }
    }
}

}  // namespace

int main() {
    offenderWordChecks();
    lastAtMostChecks();
    offsetsBadChecks();
    std::printf("ok\n");
    return 0;
}

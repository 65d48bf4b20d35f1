// The distribution and the draw of rpvg_amd/csrc/gibbs_streams.hpp against libstdc++ on the CPU: the construction of a
// std::discrete_distribution<uint32_t> (sum, quotients, partial sums, last one 1.0) and 1 000 draws each from a std::mt19937 —
// indices and generator positions —, the block recurrence the draw kernel takes in three steps, and the standard's check value.
// Built by tests/test_independent_model.py with AddressSanitizer and UBSan; prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gibbs_streams.hpp"

using namespace rpvg_streams;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

// the words of a generator, handed out from its next 624 outputs on as the draw kernel sees them: untempered state, advanced a block
// at a time through mtBlockWord
struct BlockStream {
    uint32_t x[kMtWords];
    uint32_t at = 0;
    uint64_t taken = 0;
    explicit BlockStream(std::mt19937 ahead) {
        for (uint32_t i = 0; i < kMtWords; ++i) x[i] = mtUntemper(static_cast<uint32_t>(ahead()));
    }
    uint32_t next() {
        if (at == kMtWords) {
            // step 1, 2, 3: every step reads the old words (and the new ones of earlier steps) before it writes
            const uint32_t bounds[4] = {0, kMtTail, 2 * kMtTail, kMtWords};
            for (int step = 0; step < 3; ++step) {
                uint32_t fresh[kMtWords];
                for (uint32_t i = bounds[step]; i < bounds[step + 1]; ++i) fresh[i] = mtBlockWord(x, i);
                for (uint32_t i = bounds[step]; i < bounds[step + 1]; ++i) x[i] = fresh[i];
            }
            at = 0;
        }
        ++taken;
        return mtTemper(x[at++]);
    }
};

static void compare(const std::vector<double> & weights, const uint32_t seed, const uint32_t discard, const uint32_t draws) {
    std::mt19937 reference(seed);
    reference.discard(discard);
    BlockStream stream(reference);
    std::discrete_distribution<uint32_t> distribution(weights.begin(), weights.end());
    const uint32_t n = static_cast<uint32_t>(weights.size());
    std::vector<double> cp(n, -1.0);
    const bool has = discretePartialSums([&](const uint32_t i) { return weights[i]; }, n, [&](const uint32_t i, const double v) { cp[i] = v; });
    CHECK(has == (n >= 2));
    if (has) {
        // the probabilities libstdc++ holds are the quotients; their chain is the partial sums
        const std::vector<double> p = distribution.probabilities();
        CHECK(p.size() == n);
        double run = 0.0;
        for (uint32_t i = 0; i + 1 < n; ++i) {
            run += p[i];
            CHECK(cp[i] == run);
        }
        CHECK(cp[n - 1] == 1.0);
    } else {
        for (uint32_t i = 0; i < n; ++i) CHECK(cp[i] == -1.0);
    }
    std::mt19937 positions(seed);
    positions.discard(discard);
    for (uint32_t d = 0; d < draws; ++d) {
        const uint32_t want = distribution(reference);
        uint32_t got = 0;
        if (has) {
            const uint32_t first = stream.next(), second = stream.next();
            got = discreteDraw([&](const uint32_t i) { return cp[i]; }, n, first, second);
        }
        CHECK(got == want);
    }
    // the generator's position: as many words as the header's route took
    positions.discard(stream.taken);
    CHECK(positions == reference);
    CHECK(stream.taken == (has ? 2ull * draws : 0ull));
}

int main() {
    {
        std::mt19937 standard;
        standard.discard(9999);
        CHECK(standard() == 4123659995u);  // [rand.predef]: the 10 000th output of the default-seeded generator
        BlockStream stream{std::mt19937()};
        uint32_t last = 0;
        for (int i = 0; i < 10000; ++i) last = stream.next();
        CHECK(last == 4123659995u);
    }
    const uint32_t draws = 1000;
    compare({1.0}, 1, 0, draws);                       // one weight: no draw
    compare({}, 1, 0, draws);
    compare({0.25, 0.75}, 2, 0, draws);
    compare({0.3, 0.7}, 3, 600, draws);                // across block ends, from a generator in mid-block
    compare({0.5, 0.25, 0.25, 0.0, 0.0, 0.0}, 4, 17, draws);  // late losers: exact zeros at the end
    compare({0.2, 0.0, 0.3, 0.0, 0.5}, 5, 623, draws); // zeros in the middle
    compare({0.0, 0.0, 1.0}, 6, 624, draws);
    compare({0.1, 0.2, 0.3, 0.4}, 7, 0, 312);          // exactly one block
    compare({0.1, 0.2, 0.3, 0.4}, 7, 0, 313);          // one draw into the next
    {
        std::vector<double> wide(65536);
        std::mt19937 make(99);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (auto & w: wide) w = u(make);
        compare(wide, 8, 5, draws);
        std::vector<double> flat(65536, 1.0 / 65536);
        compare(flat, 9, 5, draws);
    }
    {
        std::vector<double> decades;
        for (int e = 0; e >= -300; e -= 3) decades.push_back(std::pow(10.0, e));
        compare(decades, 10, 1, draws);
        std::vector<double> rising(decades.rbegin(), decades.rend());
        compare(rising, 11, 1, draws);
        std::vector<double> mixed;
        for (size_t i = 0; i < decades.size(); ++i) mixed.push_back(i % 2 ? decades[i] : decades[decades.size() - 1 - i]);
        compare(mixed, 12, 1, draws);
    }
    std::printf("ok\n");
    return 0;
}

// The schedule of the collapse's segment sort (rpvg_amd/csrc/segment_sort_plan.hpp) executed on host arrays, lanes and wavefronts
// simulated: every size class, the three kinds of stage taken as the header says, the chunks and the merge rounds with their two
// buffers — against std::sort.  Plain C++17; built with -fsanitize=address,undefined.  Prints "ok".
#include "segment_sort_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace rpvg_sort;
typedef std::vector<uint64_t> Words;

static uint64_t g_stages[3];

// `n` words through the network of class `c`, as sortSegmentWords does: thread t loads the words t, t + T .., pads, holds the
// elements t E .. t E + E - 1; the image is element by element
static Words sortInClass(const uint64_t * in, const uint32_t n, const SizeClass c) {
    const uint32_t E = c.words_per_lane, T = c.waves * kWaveLanes;
    REQUIRE(T * E == c.padded && n <= c.padded && (E == 1 || E == 2 || E == 4 || E == 8));
    Words flat(T * E), before(T * E);  // word e of thread t at t E + e
    struct Rows {
        uint64_t * p;
        uint32_t E;
        uint64_t * operator[](const uint32_t t) const { return p + t * E; }
    };
    const Rows v{flat.data(), E};
    for (uint32_t t = 0; t < T; ++t) {
        for (uint32_t e = 0; e < E; ++e) v[t][e] = e * T + t < n ? in[e * T + t] : kPaddingWord;
    }
    for (uint32_t k = 2; k <= c.padded; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const StageKind kind = stageKind(j, E);
            ++g_stages[kind];
            if (kind == kInLane) {
                for (uint32_t t = 0; t < T; ++t) {
                    for (uint32_t e = 0; e < E; ++e) {
                        if (e & j) continue;
                        REQUIRE(partnerOf(t * E + e, j) == t * E + (e | j));
                        const bool swap = (v[t][e] > v[t][e | j]) == ascendingAt(t * E + e, k);
                        if (swap) std::swap(v[t][e], v[t][e | j]);
                        REQUIRE(keepsSmaller(t * E + e, k, j) == ascendingAt(t * E + e, k) && keepsSmaller(t * E + (e | j), k, j) != ascendingAt(t * E + e, k));
                    }
                }
                continue;
            }
            const uint32_t d = laneDistance(j, E);
            REQUIRE(d >= 1 && d < T && (d & (d - 1)) == 0);
            before = flat;  // (everybody reads the other's word of before the stage: the exchange, or the LDS behind a barrier)
            for (uint32_t t = 0; t < T; ++t) {
                const uint32_t other = t ^ d;
                REQUIRE((kind == kInWave) == (other / kWaveLanes == t / kWaveLanes));
                for (uint32_t e = 0; e < E; ++e) {
                    REQUIRE(partnerOf(t * E + e, j) == other * E + e);
                    REQUIRE(keepsSmaller(t * E + e, k, j) == keepsSmaller(t * E, k, j));  // one predicate per lane
                    const uint64_t x = before[t * E + e], y = before[other * E + e];
                    v[t][e] = keepsSmaller(t * E + e, k, j) ? std::min(x, y) : std::max(x, y);
                }
            }
        }
    }
    Words image(c.padded);
    for (uint32_t t = 0; t < T; ++t) {
        for (uint32_t e = 0; e < E; ++e) image[t * E + e] = v[t][e];
    }
    for (uint32_t i = n; i < c.padded; ++i) REQUIRE(image[i] == kPaddingWord);
    image.resize(n);
    return image;
}

// a whole segment: the small kernel's class, or chunks and `launched` >= mergeRoundsOf(n) rounds and the final buffer
// (network = false: the chunks by std::sort — the long segments, whose rounds are the point)
static Words sortSegment(const Words & in, const uint32_t launched, const bool network = true) {
    const uint64_t R = in.size();
    if (R == 0) return Words();
    if (R <= kSmallSortRows) {
        const SizeClass c = smallClassOf(static_cast<uint32_t>(R));
        REQUIRE(c.waves == (R <= kOneWaveRows ? 1u : kSmallSortWaves) && c.padded >= R && (c.padded == kWaveLanes || c.padded / 2 < R));
        return sortInClass(in.data(), static_cast<uint32_t>(R), c);
    }
    REQUIRE(launched >= mergeRoundsOf(R));
    Words buffer[2] = {Words(R, 0x1111111111111111ull), Words(R, 0x2222222222222222ull)};
    for (uint64_t c0 = 0; c0 < R; c0 += kChunkRows) {
        const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(kChunkRows, R - c0));
        const SizeClass c = chunkClassOf(n);
        REQUIRE(c.waves == kChunkWaves && c.padded >= n);
        Words run(in.begin() + c0, in.begin() + c0 + n);
        if (network) run = sortInClass(in.data() + c0, n, c);
        else std::sort(run.begin(), run.end());
        std::copy(run.begin(), run.end(), buffer[0].begin() + c0);
    }
    for (uint32_t round = 0; round < launched; ++round) {
        if (!roundHasWork(R, round)) continue;  // (touches no memory)
        const Words & source = buffer[sourceBuffer(round)];
        Words & target = buffer[targetBuffer(round)];
        REQUIRE(sourceBuffer(round) != targetBuffer(round));
        const uint64_t run = runLength(round);
        for (uint64_t pair0 = 0; pair0 < R; pair0 += 2 * run) {
            const uint64_t a1 = std::min(R, pair0 + run), b1 = std::min(R, pair0 + 2 * run);
            REQUIRE(std::is_sorted(source.begin() + pair0, source.begin() + a1) && std::is_sorted(source.begin() + a1, source.begin() + b1));
            std::merge(source.begin() + pair0, source.begin() + a1, source.begin() + a1, source.begin() + b1, target.begin() + pair0);  // (a lone run: copied)
        }
        std::fill(buffer[sourceBuffer(round)].begin(), buffer[sourceBuffer(round)].end(), 0x3333333333333333ull + round);  // nobody may need it again
    }
    return buffer[finalBuffer(R)];
}

static void checkSorted(const Words & in, const uint32_t extra_rounds = 0, const bool network = true) {
    Words want = in;
    std::sort(want.begin(), want.end());
    const Words got = sortSegment(in, mergeRoundsOf(in.size()) + extra_rounds, network);
    REQUIRE(got == want);
}

static std::mt19937_64 g_rng(20240607);

// n distinct words below the padding value; what: 0 random, 1 low halves only differ, 2 high halves only differ
static Words distinctWords(const uint32_t n, const int what) {
    Words w(n);
    std::vector<uint32_t> part(n);
    for (uint32_t i = 0; i < n; ++i) part[i] = i * 2654435761u + 12345u;  // (odd multiplier: distinct)
    for (uint32_t i = 0; i < n; ++i) {
        if (what == 1) w[i] = 0x0123456700000000ull | part[i];
        else if (what == 2) w[i] = (static_cast<uint64_t>(part[i]) << 32) | 0x89ABCDEFu;
        else w[i] = (g_rng() & ~0xFFFFFull) | i;  // the element number in the low bits: distinct
    }
    std::shuffle(w.begin(), w.end(), g_rng);
    for (uint64_t & x : w) REQUIRE(x != kPaddingWord);
    return w;
}

static void checkLength(const uint32_t n) {
    for (int what = 0; what < 3; ++what) {
        Words w = distinctWords(n, what);
        checkSorted(w);
        if (n > 0 && what == 0) {  // the largest word a segment can hold, next to the padding
            w[g_rng() % n] = kPaddingWord - 1;
            checkSorted(w);
        }
        std::sort(w.begin(), w.end());
        checkSorted(w);
        Words organ(n);  // ascending on the even places from the left, descending on the odd ones from the right
        for (uint32_t i = 0; i < n; ++i) organ[i % 2 == 0 ? i / 2 : n - 1 - i / 2] = w[i];
        checkSorted(organ);
        std::reverse(w.begin(), w.end());
        checkSorted(w);
    }
}

int main() {
    // the classes
    REQUIRE(kOneWaveRows == 512 && kSmallSortRows == 1024 && kChunkRows == 2048 && kMaxSegmentRows == (1ull << kRowBits) - 1);
    REQUIRE((smallClassOf(1) == SizeClass{64, 1, 1}) && (smallClassOf(64) == SizeClass{64, 1, 1}) && (smallClassOf(65) == SizeClass{128, 2, 1}));
    REQUIRE((smallClassOf(128) == SizeClass{128, 2, 1}) && (smallClassOf(129) == SizeClass{256, 4, 1}) && (smallClassOf(256) == SizeClass{256, 4, 1}));
    REQUIRE((smallClassOf(257) == SizeClass{512, 8, 1}) && (smallClassOf(512) == SizeClass{512, 8, 1}) && (smallClassOf(513) == SizeClass{1024, 8, 2}));
    REQUIRE((smallClassOf(1024) == SizeClass{1024, 8, 2}));
    REQUIRE((chunkClassOf(1) == SizeClass{256, 1, 4}) && (chunkClassOf(256) == SizeClass{256, 1, 4}) && (chunkClassOf(257) == SizeClass{512, 2, 4}));
    REQUIRE((chunkClassOf(1024) == SizeClass{1024, 4, 4}) && (chunkClassOf(1025) == SizeClass{2048, 8, 4}) && (chunkClassOf(2048) == SizeClass{2048, 8, 4}));
    // the stages of the largest classes by kind: 512 words on one wavefront never leave it, 1 024 on two cross once, a chunk
    // three times (of 45, 55 and 66 stages)
    g_stages[0] = g_stages[1] = g_stages[2] = 0;
    checkSorted(distinctWords(512, 0));
    REQUIRE(g_stages[kAcrossWaves] == 0 && g_stages[kInLane] + g_stages[kInWave] == 45 && g_stages[kInWave] == 21);
    g_stages[0] = g_stages[1] = g_stages[2] = 0;
    checkSorted(distinctWords(1024, 0));
    REQUIRE(g_stages[kAcrossWaves] == 1 && g_stages[0] + g_stages[1] + g_stages[2] == 55);
    g_stages[0] = g_stages[1] = g_stages[2] = 0;
    checkSorted(distinctWords(2048, 0));
    REQUIRE(g_stages[kAcrossWaves] == 3 && g_stages[0] + g_stages[1] + g_stages[2] == 66);

    for (uint32_t n : {0u, 1u, 2u, 3u}) checkLength(n);
    for (uint32_t edge : {64u, 128u, 256u, 512u, 1024u, kChunkRows}) {
        for (uint32_t n : {edge - 1, edge, edge + 1}) checkLength(n);
    }
    // short last chunks of every chunk class
    for (uint32_t tail : {1u, 255u, 256u, 257u, 512u, 513u, 1024u, 1025u, 2047u}) checkSorted(distinctWords(kChunkRows + tail, 0));

    // the rounds: 1 .. 9 chunks and 2^k +- 1 chunks up to the row limit, full and partial last chunks, with as many rounds
    // launched as the segment needs and with up to three more (the host launches by the largest segment)
    std::vector<uint64_t> chunk_counts = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    for (uint32_t k = 4; (1ull << k) * kChunkRows <= kMaxSegmentRows + 1; ++k) {
        chunk_counts.push_back((1ull << k) - 1);
        chunk_counts.push_back(1ull << k);
        chunk_counts.push_back((1ull << k) + 1);
    }
    for (const uint64_t chunks : chunk_counts) {
        for (const uint64_t rows : {chunks * kChunkRows, chunks * kChunkRows - 7, (chunks - 1) * kChunkRows + 1}) {
            if (rows == 0 || rows > kMaxSegmentRows) continue;
            // the rounds by a direct count: runs halve, rounding up, until one is left
            uint32_t rounds = 0;
            for (uint64_t runs = chunksOf(rows); runs > 1; runs = (runs + 1) / 2) ++rounds;
            REQUIRE(chunksOf(rows) == (rows + kChunkRows - 1) / kChunkRows);
            REQUIRE(mergeRoundsOf(rows) == rounds && finalBuffer(rows) == (rounds & 1));
            for (uint32_t round = 0; round < rounds + 3; ++round) REQUIRE(roundHasWork(rows, round) == (round < rounds));
            if (rows <= kSmallSortRows) continue;
            const bool large = chunks > 9;
            Words w(large ? rows : 0);
            for (uint64_t i = 0; i < w.size(); ++i) w[i] = (i + 1) * 0x9E3779B97F4A7C15ull;  // (an odd multiplier: distinct, in no order)
            if (!large) w = distinctWords(static_cast<uint32_t>(rows), 0);
            if (chunks > 33 && rows != chunks * kChunkRows - 7) continue;  // (the longest: one length per count of chunks)
            for (uint32_t extra = 0; extra < (chunks > 33 ? 1u : large ? 2u : 4u); ++extra) checkSorted(w, extra, !large);
        }
    }
    REQUIRE(mergeRoundsOf(kMaxSegmentRows) == 9 && mergeRoundsOf(0) == 0 && mergeRoundsOf(kChunkRows) == 0 && mergeRoundsOf(kChunkRows + 1) == 1);
    std::printf("ok\n");
    return 0;
}

// The schedule of the segment sort at the head of the row collapse (row_collapse.hip, stage 0) as data: the size classes, the
// kind, partner and direction of every stage of the bitonic network, the chunk length, the merge rounds a segment needs and
// the buffer its sorted words end in — plain C++17, so that a CPU test executes the same schedule on host arrays
// (tests/cpp/segment_sort_check.cpp).  The kernels read it; nothing here knows a HIP type.
#ifndef RPVG_SEGMENT_SORT_PLAN_HPP
#define RPVG_SEGMENT_SORT_PLAN_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define RPVG_SORT_FN __host__ __device__ inline
#else
#define RPVG_SORT_FN inline
#endif

namespace rpvg_sort {

constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kMaxWordsPerLane = 8;
constexpr uint32_t kOneWaveRows = kWaveLanes * kMaxWordsPerLane;   // segments up to here: ONE wavefront, no workgroup barrier
constexpr uint32_t kSmallSortWaves = 2;                            // wavefronts of a workgroup of the small kernel
constexpr uint32_t kSmallSortRows = kSmallSortWaves * kOneWaveRows;  // segments up to here are sorted in one go; longer ones in chunks
constexpr uint32_t kChunkWaves = 4;
constexpr uint32_t kChunkRows = kChunkWaves * kWaveLanes * kMaxWordsPerLane;  // 2 048: a sorted run in front of the merge rounds
constexpr uint32_t kRowBits = 20;                                   // rows of a segment a packed word can tell apart
constexpr uint64_t kMaxSegmentRows = (1ull << kRowBits) - 1;        // longer segments take the library sort
constexpr uint64_t kPaddingWord = ~0ull;                           // behind every word a segment can hold

// A size class: `waves` wavefronts hold `padded` words, `words_per_lane` CONSECUTIVE ones per lane — lane l of the group
// (0 .. 64 waves - 1) has the elements l E .. l E + E - 1 of the network.
struct SizeClass {
    uint32_t padded, words_per_lane, waves;
};
RPVG_SORT_FN bool operator==(const SizeClass & x, const SizeClass & y) {
    return x.padded == y.padded && x.words_per_lane == y.words_per_lane && x.waves == y.waves;
}

// the classes of `waves` wavefronts: E = 1, 2, 4, 8 words per lane
RPVG_SORT_FN SizeClass classOfGroup(const uint32_t rows, const uint32_t waves) {
    uint32_t E = 1;
    while (E < kMaxWordsPerLane && rows > waves * kWaveLanes * E) E <<= 1;
    return SizeClass{waves * kWaveLanes * E, E, waves};
}
// a segment of 1 .. kSmallSortRows rows: one wavefront up to 512 rows (padded to 64, 128, 256, 512), two for 513 .. 1 024
RPVG_SORT_FN SizeClass smallClassOf(const uint32_t rows) {
    return rows <= kOneWaveRows ? classOfGroup(rows, 1) : SizeClass{kSmallSortRows, kMaxWordsPerLane, kSmallSortWaves};
}
// a chunk of 1 .. kChunkRows rows (the last chunk of a segment may be short): always the chunk kernel's four wavefronts
RPVG_SORT_FN SizeClass chunkClassOf(const uint32_t rows) { return classOfGroup(rows, kChunkWaves); }

// Stage (k, j) of the network over `padded` elements, k = 2, 4 .. padded, j = k / 2, k / 4 .. 1: element i meets element i ^ j;
// the pair ends ascending where bit k of i is clear.
enum StageKind { kInLane = 0, kInWave = 1, kAcrossWaves = 2 };
RPVG_SORT_FN StageKind stageKind(const uint32_t j, const uint32_t words_per_lane) {
    return j < words_per_lane ? kInLane : j < kWaveLanes * words_per_lane ? kInWave : kAcrossWaves;
}
RPVG_SORT_FN uint32_t partnerOf(const uint32_t i, const uint32_t j) { return i ^ j; }
RPVG_SORT_FN bool ascendingAt(const uint32_t i, const uint32_t k) { return (i & k) == 0; }
// whether element i keeps the smaller word of its pair in stage (k, j)
RPVG_SORT_FN bool keepsSmaller(const uint32_t i, const uint32_t k, const uint32_t j) { return ((i & j) == 0) == ascendingAt(i, k); }
// lanes between the two lanes of a pair (stages that are not in-lane): the lane's partner is lane ^ laneDistance
RPVG_SORT_FN uint32_t laneDistance(const uint32_t j, const uint32_t words_per_lane) { return j / words_per_lane; }

// ---- the merge behind the chunk sort ------------------------------------------------------------------------------------------
// Round r merges the runs of kChunkRows << r words of a segment two by two, from buffer r & 1 into buffer (r + 1) & 1 (buffer 0
// is the one the chunk sort writes).  A segment takes part in the rounds r < mergeRoundsOf(rows) only; in those, a last run
// without a partner is copied, so that every run of a segment that still has a round in front of it lies in the same buffer.
RPVG_SORT_FN uint32_t chunksOf(const uint64_t rows) { return static_cast<uint32_t>((rows + kChunkRows - 1) / kChunkRows); }
RPVG_SORT_FN uint32_t mergeRoundsOf(const uint64_t rows) {
    const uint64_t chunks = (rows + kChunkRows - 1) / kChunkRows;
    uint32_t rounds = 0;
    while ((1ull << rounds) < chunks) ++rounds;
    return rounds;
}
RPVG_SORT_FN uint64_t runLength(const uint32_t round) { return static_cast<uint64_t>(kChunkRows) << round; }
RPVG_SORT_FN bool roundHasWork(const uint64_t rows, const uint32_t round) { return round < mergeRoundsOf(rows); }
// the buffer (0 or 1) a round reads / writes, and the one in which the sorted words of a segment end
RPVG_SORT_FN uint32_t sourceBuffer(const uint32_t round) { return round & 1; }
RPVG_SORT_FN uint32_t targetBuffer(const uint32_t round) { return (round + 1) & 1; }
RPVG_SORT_FN uint32_t finalBuffer(const uint64_t rows) { return mergeRoundsOf(rows) & 1; }

}  // namespace rpvg_sort

#endif

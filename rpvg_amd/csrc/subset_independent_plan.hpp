// What the host decides before rpvg_hip_nested_independent_subset_em (subset_independent.hip) queues anything, as plain C++17:
// NestedPathAbundanceEstimator::inferAbundancesIndependentGroups (src/path_abundance_estimator.cpp:356-426) draws
// S = floor(1 / min_hap_prob) samples per transcript and cluster from the cluster's std::mt19937 and gives every sample the weight
// 1 / S.  The number of samples, the words a cluster takes from its generator, the capacities per cluster, the weight of a subset
// that c samples produced, and what the call refuses are all here; tests/cpp/subset_independent_plan_check.cpp runs them on the host.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "subset_full_plan.hpp"

namespace rpvg_subset_independent {

constexpr uint32_t kMaxGroupSize = rpvg_subset_full::kMaxGroupSize;
constexpr uint32_t kMaxSamples = 1024;               // min_hap_prob >= 1 / 1024: the samples of a cluster are sorted in LDS
constexpr uint64_t kMaxTranscriptSets = 65536;       // sets of one transcript: one wavefront adds its sums as one chain
constexpr uint32_t kStateWords = 624;                // std::mt19937::state_size: the words of one block of the stream
constexpr uint32_t kWordsPerDraw = 2;                // generate_canonical<double, 53> over a 32-bit generator
constexpr uint64_t kMaxWorkBytes = uint64_t(16) << 30;  // draws and sample lists of one call (device memory)

// S: the samples of every cluster, computed in double as the reference does (:364).  0 when min_hap_prob is not in (0, 1].
inline uint32_t numSamples(const double min_hap_prob) {
    if (!(min_hap_prob > 0.0) || !(min_hap_prob <= 1.0)) return 0;
    const double samples = std::floor(1 / min_hap_prob);
    return samples > 4294967295.0 ? 0xffffffffu : static_cast<uint32_t>(samples);
}

// The words a cluster takes: two per sample and transcript with at least two sets (a distribution of fewer draws nothing).  The
// number of such transcripts is known on the device only; with every transcript drawing this is the bound the host reserves by.
inline uint64_t wordsConsumed(const uint32_t samples, const uint64_t drawing_transcripts) {
    return static_cast<uint64_t>(kWordsPerDraw) * samples * drawing_transcripts;
}

// blocks of 624 words the stream kernel walks for that many words (the first one is the caller's generator_words)
inline uint64_t streamBlocks(const uint64_t words) { return (words + kStateWords - 1) / kStateWords; }

// does the generator get its state back (words >= 624), or is it moved by discard()?
inline bool stateReturned(const uint64_t words) { return words >= kStateWords; }

struct ClusterCapacity {
    uint64_t samples, subsets, path_slots, words_bound;
};
inline ClusterCapacity clusterCapacity(const uint32_t samples, const uint64_t transcripts, const uint32_t group_size) {
    return {samples, samples, static_cast<uint64_t>(samples) * transcripts * group_size, wordsConsumed(samples, transcripts)};
}

// The weight of a subset that `count` samples produced: the reference adds 1 / double(S) once per sample (:421), so it is the
// chain of `count` additions from 0.0 and not count / S.  table[0 .. S]; table[c] is the weight at c samples.
inline void weightTable(const uint32_t samples, double * table) {
    const double step = 1 / static_cast<double>(samples);
    double weight = 0.0;
    table[0] = weight;
    for (uint32_t c = 1; c <= samples; ++c) {
        weight += step;
        table[c] = weight;
    }
}

enum Refusal { kTaken = 0, kGroupSize, kDisabled, kMinHapProb, kNoGroupIds, kNoSet, kTooManySets, kTooWide, kCapacity };

struct CallShape {
    uint32_t group_size = 0;
    double min_hap_prob = 0;
    uint32_t num_matrices = 0;
    const uint32_t * columns = nullptr;   // [M] columns (paths) of every transcript
    uint32_t max_paths = 0;               // paths of the widest cluster
    bool has_group_ids = false, disabled = false;
};

// What needs no device to refuse, in the order the call names it; *which: the first offending matrix.
inline Refusal refusal(const CallShape & c, uint32_t * which) {
    if (c.group_size == 0 || c.group_size > kMaxGroupSize) return kGroupSize;
    if (c.disabled) return kDisabled;
    if (!(c.min_hap_prob * kMaxSamples >= 1.0) || !(c.min_hap_prob <= 1.0)) return kMinHapProb;
    if (!c.has_group_ids) return kNoGroupIds;
    uint64_t work_bytes = 0;
    for (uint32_t m = 0; m < c.num_matrices; ++m) {
        if (c.columns[m] == 0) {
            if (which) *which = m;
            return kNoSet;
        }
        if (rpvg_subset_full::setCount(c.columns[m], c.group_size) > kMaxTranscriptSets) {
            if (which) *which = m;
            return kTooManySets;
        }
    }
    if (c.num_matrices > 0 && !rpvg_subset_full::emVectorsFit(c.max_paths)) return kTooWide;
    // draws (4 bytes) and list entries (4 bytes each) of every sample of every transcript
    work_bytes = static_cast<uint64_t>(numSamples(c.min_hap_prob)) * c.num_matrices * 4 * (1 + static_cast<uint64_t>(c.group_size));
    if (work_bytes > kMaxWorkBytes) return kCapacity;
    return kTaken;
}

inline const char * refusalText(const Refusal r) {
    switch (r) {
        case kTaken: return "taken";
        case kGroupSize: return "group size outside 1 .. 8";
        case kDisabled: return "RPVG_HIP_NO_DEVICE_SUBSETS";
        case kMinHapProb: return "min_hap_prob outside [1/1024, 1]";
        case kNoGroupIds: return "the batch was uploaded without path_group_id: the merge needs the transcript of every path";
        case kNoSet: return "a matrix without a column has no set";
        case kTooManySets: return "a transcript with more than 65536 sets: one wavefront adds its sums as one chain";
        case kTooWide: return "a cluster too wide for LDS-resident EM vectors";
        case kCapacity: return "the draws and sample lists outgrow the memory reserved for them";
    }
    return "";
}

}  // namespace rpvg_subset_independent

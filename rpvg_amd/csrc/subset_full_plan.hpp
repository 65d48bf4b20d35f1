// The host-side arithmetic of rpvg_hip_nested_full_subset_em (subset_full.hip) and the layout of the block both nested calls
// bring back (subset_em.hip, subset_full.hip), as plain C++17: what a call may take, how a batch is cut into launches, how many
// retained sets a matrix can have, where every array sits in the packed block, and the map from a set's rank to its members.
// The kernels include the same functions (RPVG_PLAN_HD); tests/cpp/subset_full_plan_check.cpp runs them on the host.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RPVG_PLAN_HD __host__ __device__
#else
#define RPVG_PLAN_HD
#endif

namespace rpvg_subset_full {

constexpr uint32_t kMaxGroupSize = 8;
constexpr uint32_t kMaxSlots = 1024;                          // retained sets a matrix can have: posteriors sum to one, 1 / min_hap_prob of them at most
constexpr uint64_t kSetsPerLaunch = uint64_t(1) << 27;        // sets of one enumeration launch (a larger problem alone), as rpvg_hip_group_full_posteriors
constexpr uint64_t kMaxSets = 0x7fffffffull;                  // RPVG_HIP_FULL_MAX_SETS
constexpr uint64_t kEmLdsBytes = 156 * 1024;                  // em_sparse.hip, emLdsBytes: the streamed kernel's vectors

// C(n, k), k <= 8, for values that count sets of one problem (at most kMaxSets): the running product stays below 2^63.
RPVG_PLAN_HD inline uint64_t binomial(const uint64_t n, const uint32_t k) {
    if (k > n) return 0;
    uint64_t r = 1;
    for (uint32_t j = 1; j <= k; ++j) r = r * (n - k + j) / j;
    return r;
}

// Multisets of group_size out of `columns`: C(columns + group_size - 1, group_size); UINT64_MAX when it does not fit.
inline uint64_t setCount(const uint32_t columns, const uint32_t group_size) {
    if (columns == 0) return 0;
    if (group_size == 0) return 1;
    const unsigned __int128 n = static_cast<unsigned __int128>(columns) + group_size - 1;
    unsigned __int128 r = 1;
    for (uint32_t j = 1; j <= group_size; ++j) {
        r = r * (n - group_size + j) / j;
        if (r > static_cast<unsigned __int128>(UINT64_MAX)) return UINT64_MAX;
    }
    return static_cast<uint64_t>(r);
}

// The members (non-decreasing columns) of the set with lexicographic rank `rank` among the multisets of group_size out of
// `columns`: the combination b_i = member_i + i of columns + group_size - 1 through the combinatorial number system.
RPVG_PLAN_HD inline void unrankSet(const uint32_t columns, const uint32_t group_size, uint64_t rank, uint32_t * members) {
    const uint64_t n = static_cast<uint64_t>(columns) + group_size - 1;
    uint64_t x = 0;
    for (uint32_t i = 0; i < group_size; ++i) {
        if (i + 1 == group_size) {  // one set per value of the last member: no walk (a one-column-per-set problem has 2^31 of them)
            x += rank;
            rank = 0;
        }
        for (; i + 1 < group_size && x < n; ++x) {
            const uint64_t c = binomial(n - 1 - x, group_size - 1 - i);
            if (rank < c) break;
            rank -= c;
        }
        members[i] = static_cast<uint32_t>(x - i);
        ++x;
    }
}

// ... and back (the check's round trip; the enumeration kernel forms ranks the same way)
RPVG_PLAN_HD inline uint64_t rankOfSet(const uint32_t columns, const uint32_t group_size, const uint32_t * members) {
    const uint64_t n = static_cast<uint64_t>(columns) + group_size - 1;
    uint64_t rank = 0, x = 0;
    for (uint32_t i = 0; i < group_size; ++i) {
        const uint64_t b = static_cast<uint64_t>(members[i]) + i;
        for (; x < b; ++x) rank += binomial(n - 1 - x, group_size - 1 - i);
        ++x;
    }
    return rank;
}

inline uint64_t slotsOf(const uint64_t sets) { return sets < kMaxSlots ? sets : kMaxSlots; }

// The problems of one launch, [first, return): up to kSetsPerLaunch sets, a larger problem alone.  A problem is never split.
inline uint32_t chunkEnd(const uint64_t * sets, const uint32_t first, const uint32_t num_problems) {
    uint32_t end = first;
    uint64_t launch_sets = 0;
    while (end < num_problems && (end == first || launch_sets + sets[end] <= kSetsPerLaunch)) launch_sets += sets[end++];
    return end;
}

// LDS-resident EM vectors (abundances and an accumulator vector per wavefront of the streamed kernel)
inline bool emVectorsFit(const uint32_t max_paths) { return 8ull * (5ull * (static_cast<uint64_t>(max_paths) + 1) + 6) <= kEmLdsBytes; }

enum Refusal { kTaken = 0, kGroupSize, kMinHapProb, kTooManySets, kTooWide, kNoGroupIds, kDisabled };

struct CallShape {
    uint32_t group_size = 0;
    double min_hap_prob = 0;
    uint32_t num_matrices = 0;
    const uint32_t * columns = nullptr;   // [M]
    uint32_t max_paths = 0;               // paths of the widest cluster
    bool has_group_ids = false, disabled = false;
};

// What needs no device to refuse, in the order the call names it; *which: the first matrix over the set bound.
inline Refusal refusal(const CallShape & c, uint32_t * which) {
    if (c.group_size == 0 || c.group_size == 2 || c.group_size > kMaxGroupSize) return kGroupSize;
    if (c.disabled) return kDisabled;
    if (!(c.min_hap_prob * kMaxSlots >= 1.0)) return kMinHapProb;
    if (!c.has_group_ids) return kNoGroupIds;
    for (uint32_t m = 0; m < c.num_matrices; ++m) {
        if (setCount(c.columns[m], c.group_size) > kMaxSets) {
            if (which) *which = m;
            return kTooManySets;
        }
    }
    if (c.num_matrices > 0 && !emVectorsFit(c.max_paths)) return kTooWide;
    return kTaken;
}

// The results of a nested call as ONE block (device, then page-locked host memory): every array 64-byte aligned, in this order.
// (A D2H copy costs the stream ~40 us next to running kernels whatever its size: twelve arrays were 0.5 ms at the end of
// every lane.)  M matrices, S subsets, L list entries, C columns.  group_size 0 is the diploid call (set_first / set_second, two
// abundances per set slot); group_size g > 0 the full-enumeration call: g members and g abundances per set slot, the set sizes,
// and the R retained sets behind them.
struct PackedLayout {
    size_t subset_off, weight, path_off, col_off, abundances, noise, total, path, col_path, iterations, kept_rows, kept_entries, bytes;
    // the posterior-weighted merge: per matrix the number of path group sets and the noise count, per set (the sets of matrix m from
    // slot path_off[subset_off[m]] on: a matrix has at most as many as its subsets list paths) its paths, its posterior and the
    // abundance of every path; flags[0]: a transcript with more paths in one subset than a set holds
    size_t set_count, cluster_noise, set_first, set_second, set_posterior, set_abund, merge_flags;
    size_t set_size, set_member, retained_off, retained_rank, retained_posterior;  // group_size > 0 only
};
RPVG_PLAN_HD inline PackedLayout packedLayout(const uint64_t M, const uint64_t S, const uint64_t L, const uint64_t C, const uint32_t group_size = 0,
                                              const uint64_t R = 0) {
    PackedLayout p;
    size_t at = 0;
    auto place = [&](const size_t bytes) {
        const size_t here = at;
        at += (bytes + 63) & ~static_cast<size_t>(63);
        return here;
    };
    p.subset_off = place((M + 1) * 8);
    p.weight = place(S * 8);
    p.path_off = place((S + 1) * 8);
    p.col_off = place((S + 1) * 8);
    p.abundances = place(C * 8);
    p.noise = place(S * 8);
    p.total = place(S * 8);
    p.path = place(L * 4);
    p.col_path = place(C * 4);
    p.iterations = place(S * 4);
    p.kept_rows = place(S * 4);
    p.kept_entries = place(S * 4);
    p.set_count = place(M * 4);
    p.cluster_noise = place(M * 8);
    if (group_size == 0) {
        p.set_first = place(L * 4);
        p.set_second = place(L * 4);
        p.set_posterior = place(L * 8);
        p.set_abund = place(L * 16);
        p.merge_flags = place(64);
        p.set_size = p.set_member = p.retained_off = p.retained_rank = p.retained_posterior = at;
    } else {
        p.set_first = p.set_second = at;
        p.set_posterior = place(L * 8);
        p.set_abund = place(L * 8 * group_size);
        p.merge_flags = place(64);
        p.set_size = place(L * 4);
        p.set_member = place(L * 4 * group_size);
        p.retained_off = place((M + 1) * 8);
        p.retained_rank = place(R * 8);
        p.retained_posterior = place(R * 8);
    }
    p.bytes = at;
    return p;
}

}  // namespace rpvg_subset_full

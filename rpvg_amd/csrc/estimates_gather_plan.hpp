// The rules of the gather of resident estimates (estimates_gather.hip; interface include/rpvg_table.h, rpvg_estimates_part) as plain
// C++17 under the RPVG_PLAN_FN convention: the size, the members and the abundances of a set slot in both forms of a part, the
// validations in their reporting order, and gatherModel — the whole gather as one host loop over parts in host memory.  The kernels
// include this header for the rules, so each exists once; tests/cpp/estimates_gather_plan_check.cpp runs them on the host.
//
// A part has U units (matrices of the collapsed nested calls, clusters of the independent one), S path subsets and L list entries
// (= set slots).  The merged sets of unit u sit in the slots first + q, first = path_off[subset_off[u]], q < set_count[u], and the
// unit has path_off[subset_off[u + 1]] - first slots.
//   width 0      set_first, set_second (kNoMember: one path), two abundance cells per slot
//   width 1..8   set_size, set_member and set_abundance with `width` cells per slot
// The gather copies: nothing in this file executes a floating-point operation.
#ifndef RPVG_HIP_ESTIMATES_GATHER_PLAN_HPP
#define RPVG_HIP_ESTIMATES_GATHER_PLAN_HPP

#include <cstdint>
#include <vector>

#include "table_kit.hpp"

namespace rpvg_gather {

using rpvg_hip_detail::word64;

constexpr uint32_t kMaxWidth = 8;
constexpr uint32_t kNoMember = 0xffffffffu;
constexpr uint64_t kMaxSets = (1ull << 30) - 1, kMaxItems = 0x7fffffffull;  // of one rpvg_estimates_flat (rpvg_table.h)

// a part with pointers its reader can follow (the kernels: device memory; gatherModel: host memory)
struct Part {
    uint32_t num_units = 0, width = 0;
    uint64_t num_subsets = 0, num_slots = 0;
    const uint64_t * subset_off = nullptr;         // [U+1]
    const uint64_t * path_off = nullptr;           // [S+1]
    const uint32_t * set_count = nullptr;          // [U]
    const double * cluster_noise_count = nullptr;  // [U]
    const double * set_posterior = nullptr;        // [L]
    const uint32_t * set_first = nullptr, * set_second = nullptr;  // [L] width 0
    const uint32_t * set_size = nullptr;           // [L] width > 0
    const uint32_t * set_member = nullptr;         // [L x width]
    const double * set_abundance = nullptr;        // [L x cellsPerSlot]
};

// ---- a slot in both forms -------------------------------------------------------------------------------------------------
RPVG_PLAN_FN uint32_t cellsPerSlot(const uint32_t width) { return width == 0 ? 2u : width; }
// the most members a set of the form can have: all of its cells (a size beyond them would be read from the next slot)
RPVG_PLAN_FN uint32_t maxSetSize(const uint32_t width) { return cellsPerSlot(width); }

// the size as the part states it: validated by slotOffence before a member is read
RPVG_PLAN_FN uint32_t slotSize(const Part & p, const uint64_t slot) {
    return p.width == 0 ? (p.set_second[slot] == kNoMember ? 1u : 2u) : p.set_size[slot];
}
RPVG_PLAN_FN uint32_t slotMember(const Part & p, const uint64_t slot, const uint32_t j) {
    return p.width == 0 ? (j == 0 ? p.set_first[slot] : p.set_second[slot]) : p.set_member[slot * p.width + j];
}
RPVG_PLAN_FN double slotAbundance(const Part & p, const uint64_t slot, const uint32_t j) { return p.set_abundance[slot * cellsPerSlot(p.width) + j]; }

// ---- the validations, in their reporting order ------------------------------------------------------------------------------
// The offender word (table_kit.hpp) of a unit's offence is offenderWord(g, why) with g the unit's index over all parts (the units of
// part 0, then those of part 1, ...): the minimum is the smallest offending (part, unit) and, of its offences, the first of this list.
// A width above kMaxWidth is an offence of the part (second kind, index = the part) and is looked for before any unit is.
enum GatherBad {
    kBadUnitCluster = 1,  // unit_cluster >= K
    kBadDuplicate = 2,    // the cluster is listed by another unit as well (every unit that shares its cluster offends)
    kBadSubsetOff = 3,    // offsetsBad(subset_off, u, U, S)
    kBadPathOff = 4,      // offsetsBad(path_off, s, S, L) for a subset s of the unit
    kBadSetCount = 5,     // set_count[u] beyond the unit's slots
    kBadSetSize = 6,      // a set size outside 1 .. maxSetSize(width)
    kBadMember = 7        // a member at or beyond the cluster's number of paths
};
constexpr int kBadWidth = 1;  // (second kind)

inline const char * reasonOf(const int why) {
    static const char * const kReasons[] = {"",
                                            "unit_cluster is not below the batch's number of clusters",
                                            "its cluster is listed by two units",
                                            "subset_off is not a non-decreasing sequence of offsets from 0 to num_subsets",
                                            "path_off is not a non-decreasing sequence of offsets from 0 to num_slots",
                                            "set_count is beyond the unit's slots",
                                            "a set size is outside 1 .. the cells of a slot",
                                            "a member is not below the cluster's number of paths"};
    return why >= 1 && why <= kBadMember ? kReasons[why] : kReasons[0];
}

// the unit's subsets [s0, s1): true when subset_off fails (nothing else of the unit may be read then)
RPVG_PLAN_FN bool unitSubsetsBad(const Part & p, const uint32_t u, uint64_t * s0, uint64_t * s1) {
    if (rpvg_hip_detail::offsetsBad(p.subset_off, u, p.num_units, p.num_subsets)) return true;
    *s0 = p.subset_off[u];
    *s1 = p.subset_off[u + 1];
    return false;
}
RPVG_PLAN_FN bool subsetPathsBad(const Part & p, const uint64_t s) { return rpvg_hip_detail::offsetsBad(p.path_off, s, p.num_subsets, p.num_slots); }
// The unit's first slot and its number of slots, its subsets [s0, s1) having passed subsetPathsBad (so first <= end <= L; a unit
// without subsets has no slot and reads path_off[s0], s0 <= S, alone).
RPVG_PLAN_FN void unitSlots(const Part & p, const uint64_t s0, const uint64_t s1, uint64_t * first, uint64_t * slots) {
    *first = p.path_off[s0];
    *slots = s1 > s0 ? p.path_off[s1] - *first : 0;
}
// 0, kBadSetSize or kBadMember of one slot (below L) of a cluster of num_paths paths; *size: its size when it is valid
RPVG_PLAN_FN int slotOffence(const Part & p, const uint64_t slot, const uint64_t num_paths, uint32_t * size) {
    const uint32_t n = slotSize(p, slot);
    if (n < 1 || n > maxSetSize(p.width)) return kBadSetSize;
    for (uint32_t j = 0; j < n; ++j) {
        if (slotMember(p, slot, j) >= num_paths) return kBadMember;
    }
    *size = n;
    return 0;
}
// noise_count of a cluster with a unit: the rule of unpackMergedSolutions / unpackMergedSetSolutions
RPVG_PLAN_FN double unitNoise(const Part & p, const uint32_t u, const double cluster_total) {
    return p.subset_off[u + 1] > p.subset_off[u] ? p.cluster_noise_count[u] : cluster_total;
}

// ---- the whole gather as one host loop --------------------------------------------------------------------------------------
struct HostPart {
    Part part;
    const uint32_t * unit_cluster = nullptr;  // [U]
};

struct FlatArrays {  // rpvg_estimates_flat without the batch's two arrays
    std::vector<uint64_t> set_off, member_off, abund_off;
    std::vector<uint32_t> members;
    std::vector<double> posteriors, abundances, noise_count;
};

// The offender word of the first offence (`out` is left empty), or kNoBad and the flat arrays of the K clusters.
// cluster_path_off [K+1] and cluster_total [K] are the batch's.
inline word64 gatherModel(const uint32_t K, const uint64_t * cluster_path_off, const double * cluster_total, const HostPart * parts,
                          const uint32_t num_parts, FlatArrays & out) {
    out = FlatArrays();
    for (uint32_t p = 0; p < num_parts; ++p) {
        if (parts[p].part.width > kMaxWidth) return rpvg_hip_detail::offenderWord(p, kBadWidth, true);
    }
    std::vector<uint32_t> listed(K, 0);
    for (uint32_t p = 0; p < num_parts; ++p) {
        for (uint32_t u = 0; u < parts[p].part.num_units; ++u) {
            const uint32_t c = parts[p].unit_cluster[u];
            if (c < K && listed[c] < 2) ++listed[c];
        }
    }
    struct Owner {
        uint32_t part = 0, unit = 0;
        bool any = false;
    };
    std::vector<Owner> owner(K);
    uint64_t g = 0;
    for (uint32_t p = 0; p < num_parts; ++p) {
        const Part & part = parts[p].part;
        for (uint32_t u = 0; u < part.num_units; ++u, ++g) {
            const uint32_t c = parts[p].unit_cluster[u];
            int why = 0;
            uint64_t s0 = 0, s1 = 0;
            if (c >= K) why = kBadUnitCluster;
            else if (listed[c] > 1) why = kBadDuplicate;
            else if (unitSubsetsBad(part, u, &s0, &s1)) why = kBadSubsetOff;
            else {
                for (uint64_t s = s0; s < s1 && !why; ++s) {
                    if (subsetPathsBad(part, s)) why = kBadPathOff;
                }
            }
            if (!why) {
                uint64_t first = 0, slots = 0;
                unitSlots(part, s0, s1, &first, &slots);
                const uint64_t count = part.set_count[u], num_paths = cluster_path_off[c + 1] - cluster_path_off[c];
                if (count > slots) why = kBadSetCount;
                for (uint64_t q = 0; q < count && !why; ++q) {  // a bad size anywhere comes before a bad member anywhere
                    const uint32_t n = slotSize(part, first + q);
                    if (n < 1 || n > maxSetSize(part.width)) why = kBadSetSize;
                }
                for (uint64_t q = 0; q < count && !why; ++q) {
                    uint32_t n = 0;
                    why = slotOffence(part, first + q, num_paths, &n);
                }
            }
            if (why) return rpvg_hip_detail::offenderWord(g, why);
            owner[c].part = p;
            owner[c].unit = u;
            owner[c].any = true;
        }
    }
    out.set_off.assign(1, 0);
    out.member_off.assign(1, 0);
    out.abund_off.assign(1, 0);
    for (uint32_t k = 0; k < K; ++k) {
        double noise = cluster_total[k];
        if (owner[k].any) {
            const Part & part = parts[owner[k].part].part;
            const uint32_t u = owner[k].unit;
            uint64_t first = 0, slots = 0;
            unitSlots(part, part.subset_off[u], part.subset_off[u + 1], &first, &slots);
            for (uint64_t q = 0; q < part.set_count[u]; ++q) {
                const uint64_t slot = first + q;
                const uint32_t n = slotSize(part, slot);
                for (uint32_t j = 0; j < n; ++j) {
                    out.members.push_back(slotMember(part, slot, j));
                    out.abundances.push_back(slotAbundance(part, slot, j));
                }
                out.member_off.push_back(out.members.size());
                out.posteriors.push_back(part.set_posterior[slot]);
            }
            noise = unitNoise(part, u, cluster_total[k]);
        }
        out.set_off.push_back(out.posteriors.size());
        out.abund_off.push_back(out.abundances.size());
        out.noise_count.push_back(noise);
    }
    return rpvg_hip_detail::kNoBad;
}

}  // namespace rpvg_gather

#endif
